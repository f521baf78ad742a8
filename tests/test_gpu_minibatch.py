"""Minibatch PPO updates on the GPU: navppo_shuffle_batch against index_select by its host mirror (every row format, guarded buffers,
refusals, the gate), the minibatch update of every fused family against the same *_update_epoch entry point called step by step on
host-permuted, host-sliced contiguous copies (bit for bit), against the PyTorch path (the tolerances of
test_fused_update_tracks_pytorch_update_over_epochs, plus the step-averaged gradient norms), the early stop in the middle of an epoch,
two gloo ranks sharing the GPU against one process that plays both, and the trainer end to end."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from _guards import is_canary, ptr, run_both
from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd._native import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KEY, COUNTER = ppo.minibatch_key(5), ppo.minibatch_counter(3, 17)


# ------------------------------------------------------------------------------------------------ the shuffle kernel
def _rows(n, D, half, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    obs = torch.rand((n, D), generator=g).to(torch.float16 if half else torch.float32)
    act = torch.rand((n, 2), generator=g)
    return [obs, act] + [torch.randn(n, generator=g) for _ in range(3)]


def _obs_align(D, half):
    return 16 if D == 16 else 4 if half else 8


def _shuffle(ins, outs, D, half, n, gate=None, key=KEY, counter=COUNTER):
    rc = lib().navppo_shuffle_batch(ptr(ins[0]), D, int(half), *(ptr(t) for t in ins[1:]), n, key, counter, *(ptr(t) for t in outs), ptr(gate),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


def _place(g, host, D, half):
    """the five inputs and the five outputs of a call inside the arena `g`, each at the alignment the ABI asks of it"""
    al = (_obs_align(D, half), 8, 4, 4, 4)
    ins = [g.inp(t, a) for t, a in zip(host, al)]
    outs = [g.out(t.shape, t.dtype, a) for t, a in zip(host, al)]
    return ins, outs


@pytest.mark.parametrize("D,half", [(16, False), (16, True), (42, False), (42, True)])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 4099, 65553])
def test_shuffle_is_index_select_by_the_host_permutation(n, D, half):
    host = _rows(n, D, half)
    perm = ppo.batch_permutation(n, KEY, COUNTER)
    want = [t.index_select(0, perm) for t in host]

    def call(g):
        ins, outs = _place(g, host, D, half)
        assert _shuffle(ins, outs, D, half, n) == 0, lib().navppo_last_error().decode()
        return outs

    outs = run_both(DEV, call, f"navppo_shuffle_batch n={n} D={D} f16={half}")   # guards untouched, no canary left, both placements equal
    for got, w in zip(outs, want):
        assert torch.equal(got.cpu().view(torch.uint8), w.contiguous().view(torch.uint8))


def test_shuffle_refuses_bad_arguments_and_writes_nothing():
    n, D = 1000, 16
    host = _rows(n, D, False)

    def call(g):
        ins, outs = _place(g, host, D, False)
        bad = []
        for k in range(5):   # every output on top of its own input, and one output overlapping another input by a tail
            o = list(outs)
            o[k] = ins[k]
            bad.append(_shuffle(ins, o, D, False, n))
        shifted = ins[2][8:]   # logp_out inside logp_old_dev
        bad.append(_shuffle(ins, outs[:2] + [shifted] + outs[3:], D, False, n - 8))
        bad.append(_shuffle(ins, outs, D, False, 0))
        bad.append(_shuffle(ins, outs, D, False, 1 << 31))
        bad.append(_shuffle(ins, outs, 17, False, n))
        bad.append(_shuffle(ins, outs[:4] + [None], D, False, n))
        bad.append(_shuffle([ins[0].reshape(-1)[1:]] + ins[1:], outs, D, False, n - 1))   # an observation pointer 4 bytes off its alignment
        bad.append(_shuffle(ins, outs[:1] + [outs[1].reshape(-1)[1:]] + outs[2:], D, False, n - 1))   # act_out 4 bytes off
        assert all(rc != 0 for rc in bad), bad
        assert "navppo_shuffle_batch" in lib().navppo_last_error().decode()
        torch.cuda.synchronize()
        for t in outs:
            assert bool(is_canary(t).all())
        for t, h in zip(ins, host):
            assert torch.equal(t.cpu(), h)
        assert _shuffle(ins, outs, D, False, n) == 0   # (and the call the arena's check expects)
        return outs

    run_both(DEV, call, "navppo_shuffle_batch refusals")


def test_a_set_gate_leaves_the_outputs_alone():
    n, D = 4099, 42
    host = _rows(n, D, False)
    ins = [t.to(DEV) for t in host]
    outs = [torch.empty_like(t) for t in ins]
    for t in outs:
        t.view(torch.int32).fill_(0x7FC0DEAD)
    kept = [t.clone() for t in outs]
    gate = torch.tensor([1.0, 3.0, 0.02, 4.0], device=DEV)
    assert _shuffle(ins, outs, D, False, n, gate=gate) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, kept))
    gate.zero_()   # an open gate: the shuffle
    assert _shuffle(ins, outs, D, False, n, gate=gate) == 0
    perm = ppo.batch_permutation(n, KEY, COUNTER).to(DEV)
    assert all(torch.equal(o, t.index_select(0, perm)) for o, t in zip(outs, ins))


# ------------------------------------------------------------------------------------------------ the update against slice calls
FAMILIES = {"mlp64_f32": ("mlp64x2", "f32", 16, False), "bf16x3_16": ("mlp64x2", "bf16x3", 16, False),
            "bf16x3_42": ("mlp64x2", "bf16x3", 42, False), "bf16x3_f16": ("mlp64x2", "bf16x3", 16, True),
            "resmlp512": ("resmlp512", "bf16x3", 16, False)}
VAR = 0.6


def _updater(fam, seed=7, **cfg):
    policy, arith, D, _ = FAMILIES[fam]
    torch.manual_seed(seed)
    a, c = nets.make_policy(policy, D, 2)
    a.to(DEV), c.to(DEV)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, update_arith=arith, **cfg), None, DEV)
    assert up.fused is not None and up.bf16x3 == (policy == "mlp64x2" and arith == "bf16x3")
    return up


def _update_batch(up, fam, n, seed=21):
    """rows whose logp_old is the start policy's own log-probability of the actions: approx_kl starts at 0 and grows with every step"""
    _, _, D, half = FAMILIES[fam]
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, D), generator=g).to(torch.float16 if half else torch.float32).to(DEV)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(DEV)
    rtg = (torch.randn(n, generator=g) * 3).to(DEV)
    with torch.no_grad():
        logp = ppo.gaussian_log_prob(up.actor(obs.float()), acts, torch.tensor(VAR, device=DEV)).contiguous()
    return obs, acts, logp, rtg


def _plain_batch(fam, n, seed):
    """rows that do not depend on the nets (made on the CPU from a seeded generator: the same bits in every process)"""
    _, _, D, half = FAMILIES[fam]
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, D), generator=g).to(torch.float16 if half else torch.float32)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    return tuple(t.to(DEV) for t in (obs, acts, -1.2 - 2.3 * torch.rand(n, generator=g), torch.randn(n, generator=g) * 3))


def _host_steps(batch, adv, n_ep, size, mode, update_index=0, key=ppo.minibatch_key(0)):
    """every step's batch as contiguous copies of its own: permuted and sliced on the host"""
    n = batch[0].shape[0]
    full = tuple(batch) + (adv,)
    for ep in range(n_ep):
        if mode == "none":
            order = torch.arange(n)
        else:
            order = ppo.batch_permutation(n, key, ppo.minibatch_counter(update_index, ep if mode == "epoch" else 0))
        for lo in range(0, n, size):
            idx = order[lo:lo + size].to(DEV)
            yield tuple(t.index_select(0, idx).clone() for t in full)


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
@pytest.mark.parametrize("mode", ["epoch", "update", "none"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_minibatch_update_is_the_epoch_entry_point_on_host_slices(fam, mode, max_grad_norm):
    n, size, n_ep = 3 * 96 + 40, 96, 2
    steps = n_ep * 4
    up = _updater(fam, n_updates_per_iteration=n_ep, minibatch_size=size, minibatch_shuffle=mode, max_grad_norm=max_grad_norm)
    ref = _updater(fam, n_updates_per_iteration=n_ep, max_grad_norm=max_grad_norm)
    assert torch.equal(up.fp.flat, ref.fp.flat)
    batch = _update_batch(up, fam, n)
    with torch.no_grad():
        adv = ppo.normalise_advantages(batch[3] - ref.value(batch[0]))
    hist = torch.zeros((steps, 8), device=DEV)
    cs = torch.zeros((steps, 4), device=DEV) if max_grad_norm is not None else None
    for st, sl in enumerate(_host_steps(batch, adv, n_ep, size, mode)):
        ref.invalidate_prepared()   # (a fresh copy may reuse a freed one's address: torch's version counter does not tell them apart)
        ref._fused_epoch(*sl, VAR, hist[st], None if cs is None else cs[st])
    stats = up.update(*batch, VAR)
    torch.cuda.synchronize()
    assert up._adam_t == ref._adam_t == steps
    assert torch.equal(up.fp.flat, ref.fp.flat) and torch.equal(up._adam_m, ref._adam_m) and torch.equal(up._adam_v, ref._adam_v)
    assert torch.equal(up._fhist[:steps, [0, 1, 2, 4]], hist[:, [0, 1, 2, 4]])
    if cs is not None:
        assert up.clip_stats.shape == (steps, 4) and torch.equal(up.clip_stats, cs)
    assert up.loss_history.shape == (n_ep, 2) and all(math.isfinite(v) for v in stats.values())
    want = hist[:, [0, 4]].reshape(n_ep, 4, 2).mean(1)
    np.testing.assert_allclose(up.loss_history.cpu().numpy(), want.cpu().numpy(), rtol=1e-6)


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_a_minibatch_at_or_above_the_batch_is_the_full_batch_update(fam):
    n = 3 * 96 + 40
    res = []
    for mb in (None, 352, 1 << 20):
        up = _updater(fam, n_updates_per_iteration=3, minibatch_size=mb)
        st = up.update(*_update_batch(up, fam, n), VAR)
        res.append((up.fp.flat.clone(), up._adam_m.clone(), up._adam_v.clone(), st))
        assert up._shuf is None   # nothing new ran
    for r in res[1:]:
        assert all(torch.equal(x, y) for x, y in zip(r[:3], res[0][:3])) and r[3] == res[0][3]


# ------------------------------------------------------------------------------------------------ against the PyTorch path
@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_minibatch_update_tracks_the_pytorch_path(policy):
    """4 slices of 8192 and one of 2085, two epochs: 10 optimiser steps, the step count of
    test_fused_update_tracks_pytorch_update_over_epochs, and its tolerances; in addition the step-averaged gradient norms (rel 1e-3) -- this
    case holds the shorter last slice and the epoch boundary, where the fused epochs' squared-norm slots of the step before must not be
    misread."""
    n, size, n_ep = 4 * 8192 + 2085, 8192, 2
    g = torch.Generator().manual_seed(5)
    obs = torch.rand((n, 16), generator=g).to(DEV)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(DEV)
    logp = (-1.2 - 2.3 * torch.rand(n, generator=g)).to(DEV)
    rtg = (torch.randn(n, generator=g) * 60 + 20).to(DEV)
    res = []
    for fused in (True, False):
        torch.manual_seed(11)
        a, c = nets.make_policy(policy)
        a.to(DEV), c.to(DEV)
        up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, n_updates_per_iteration=n_ep, fused_update=fused, minibatch_size=size), None, DEV)
        assert (up.fused is not None) == fused
        st = up.update(obs, acts, logp, rtg, torch.tensor(0.8, device=DEV))
        res.append((up.fp.flat.clone(), up.loss_history.clone(), st))
    (w1, h1, s1), (w0, h0, s0) = res
    print({k: (s1[k], s0[k]) for k in s1}, float((w1 - w0).abs().max()))
    np.testing.assert_allclose(h1.cpu().numpy(), h0.cpu().numpy(), rtol=2e-4, atol=1e-5)
    assert (w1 - w0).abs().max().item() < 3e-5
    for k in ("actor_loss", "critic_loss", "approx_kl", "clip_frac"):
        assert s1[k] == pytest.approx(s0[k], rel=2e-3, abs=2e-5), k
    for k in ("grad_norm", "actor_grad_norm", "critic_grad_norm"):
        assert s1[k] == pytest.approx(s0[k], rel=1e-3), k


# ------------------------------------------------------------------------------------------------ the early stop
@pytest.mark.parametrize("fam", ["bf16x3_16", "resmlp512"])
def test_an_early_stop_in_the_second_slice_of_the_first_epoch(fam):
    n, size, n_ep = 3 * 96 + 40, 96, 3
    probe = _updater(fam, n_updates_per_iteration=1, minibatch_size=size)
    batch = _update_batch(probe, fam, n)
    probe.update(*batch, VAR)
    kl0, kl1 = (float(v) for v in probe._fhist[:2, 1])
    assert kl1 > kl0 and kl1 > 0, (kl0, kl1)   # (logp_old is the start policy's own: the first slice sees ~0, the second what one step moved)
    limit = 0.5 * (max(kl0, 0.0) + kl1)
    up = _updater(fam, n_updates_per_iteration=n_ep, minibatch_size=size, target_kl=limit / 1.5)
    ref = _updater(fam, n_updates_per_iteration=n_ep)
    with torch.no_grad():
        adv = ppo.normalise_advantages(batch[3] - ref.value(batch[0]))
    first = next(_host_steps(batch, adv, 1, size, "epoch"))
    ref._fused_epoch(*first, VAR, torch.zeros(8, device=DEV))
    st = up.update(*batch, VAR)
    torch.cuda.synchronize()
    assert st["kl_stop_step"] == 1 and st["kl_stop_epoch"] == 0 and st["kl_stopped"] == 1
    assert torch.equal(up.fp.flat, ref.fp.flat) and torch.equal(up._adam_m, ref._adam_m) and torch.equal(up._adam_v, ref._adam_v)
    assert up._adam_t == 1
    h = up.loss_history
    assert h.shape == (n_ep, 2) and bool(torch.isfinite(h[0]).all()) and bool(torch.isnan(h[1:]).all())
    assert float(up.kl_state[0]) == 1.0 and float(up.kl_state[1]) == 1.0
    assert torch.equal(up.clip_stats[1, 2:], torch.zeros(2, device=DEV))


# ------------------------------------------------------------------------------------------------ two ranks (the multi-GPU runner)
def _mb_rank_worker(rank, world, port, path, fam, n, size, n_ep):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduces here
    ctx = ppo.DistCtx(device="cuda:0")
    policy, arith, D, _ = FAMILIES[fam]
    torch.manual_seed(7)
    a, c = nets.make_policy(policy, D, 2)
    a.to(DEV), c.to(DEV)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, update_arith=arith, n_updates_per_iteration=n_ep, minibatch_size=size), ctx, DEV)
    st = up.update(*_plain_batch(fam, n, 30 + rank), VAR)
    torch.cuda.synchronize()
    torch.save({"flat": up.fp.flat.cpu(), "m": up._adam_m.cpu(), "v": up._adam_v.cpu(), "t": up._adam_t, "stats": st, "adv": up._last_adv.cpu()},
               f"{path}.{rank}")
    ctx.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("fam", ["bf16x3_16", "resmlp512"])
def test_two_ranks_equal_one_process_that_plays_both(tmp_path, fam):
    """_run_fused_multi on minibatches, two gloo ranks sharing the GPU: per step every rank's *_loss_grad on its own slice (its own
    permutation: the key mixes the rank), the all-reduced sum, navppo_adam_step at 1 / world -- against one process that makes the same
    calls for both ranks on host-permuted, host-sliced copies and adds the two gradients itself."""
    from _ranks import spawn_ranks
    n, size, n_ep, steps = 3 * 96 + 40, 96, 2, 8
    path = str(tmp_path / "mbdp")
    spawn_ranks(_mb_rank_worker, 2, lambda port: (2, port, path, fam, n, size, n_ep))
    r0, r1 = torch.load(path + ".0"), torch.load(path + ".1")
    assert all(torch.equal(r0[k], r1[k]) for k in ("flat", "m", "v")) and r0["t"] == r1["t"] == steps
    assert all(math.isfinite(v) for v in r0["stats"].values())
    ref = _updater(fam, n_updates_per_iteration=n_ep)
    batches = [_plain_batch(fam, n, 30 + r) for r in range(2)]
    with torch.no_grad():   # the advantages over both ranks' samples, from the summed moments (normalise_advantages with a context)
        raw = [b[3] - ref.value(b[0]) for b in batches]
        m = sum(torch.stack([r.double().sum(), (r.double() * r.double()).sum(), torch.tensor(float(n), dtype=torch.float64, device=DEV)])
                for r in raw)
        mean = m[0] / m[2]
        std = torch.sqrt(torch.clamp((m[1] - m[2] * mean * mean) / (m[2] - 1), min=0.0))
        advs = [(r - mean.float()) / (std.float() + 1e-10) for r in raw]
    assert torch.equal(advs[0].cpu(), r0["adv"]) and torch.equal(advs[1].cpu(), r1["adv"])
    gens = [_host_steps(batches[r], advs[r], n_ep, size, "epoch", key=ppo.minibatch_key(0, r)) for r in range(2)]
    for _ in range(steps):
        g = []
        for r in range(2):
            ref.invalidate_prepared()   # (a fresh copy may reuse the freed one's address: torch's version counter does not tell them apart)
            ref._fused_loss_grad(*next(gens[r]), VAR)
            g.append(ref.fp.grad.clone())
        ref.fp.grad.copy_(g[0] + g[1])
        ref._fused_adam(0.5)
    torch.cuda.synchronize()
    assert ref._adam_t == steps
    assert torch.equal(r0["flat"], ref.fp.flat.cpu()) and torch.equal(r0["m"], ref._adam_m.cpu()) and torch.equal(r0["v"], ref._adam_v.cpu())


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_runs_two_iterations_on_minibatches(policy):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(64, map="stage_1", max_episode_steps=12, seed=1)
    cfg = ppo.PPOConfig(rollout_len=16, max_episode_steps=12, n_updates_per_iteration=2, policy=policy, seed=2, minibatch_size=256)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.updater.fused is not None
    for it in (1, 2):
        lg = tr.iteration()
        assert lg["iteration"] == it
        for k in ("actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "actor_grad_norm", "critic_grad_norm", "value_mean"):
            assert math.isfinite(lg[k]), (k, lg[k])
    assert tr.updater._adam_t == 2 * 2 * 4 and tr.updater.update_index == 2
    assert tr.updater.loss_history.shape == (2, 2) and bool(torch.isfinite(tr.updater.loss_history).all())
    env.close()
