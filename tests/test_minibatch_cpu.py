"""PPOConfig.minibatch_size / minibatch_shuffle without a GPU: the host mirror of the device permutation (bijection, counters, mixing),
the PyTorch formulation of the minibatch update against a hand-written loop over index_select'ed slices (bit for bit; clipping; an
early stop in the middle of an epoch), validation, two gloo ranks against one process that plays both, and the full-batch identity."""
import math
import os

import numpy as np
import pytest
import torch

from navbot_ppo_amd import main as cli
from navbot_ppo_amd import nets, ppo

CPU = torch.device("cpu")
LR, CLIP = 3e-4, 0.2


# ------------------------------------------------------------------------------------------------ the permutation
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1000, 4099, 65536, 65537, 2 ** 20 + 3])
def test_batch_permutation_is_a_bijection(n):
    for key, counter in ((0, 0), (1, 5), (ppo.minibatch_key(7, 3), ppo.minibatch_counter(11, 49)), (2 ** 64 - 1, 2 ** 64 - 1)):
        p = ppo.batch_permutation(n, key, counter)
        assert p.dtype == torch.int64 and p.shape == (n,)
        assert torch.equal(torch.sort(p)[0], torch.arange(n)), (n, key, counter)
        assert torch.equal(p, ppo.batch_permutation(n, key, counter))   # a pure function of (n, key, counter)


def test_counters_keys_and_ranks_give_different_permutations():
    n, seen = 1000, []
    for u in range(3):
        for e in range(3):
            seen.append(ppo.batch_permutation(n, ppo.minibatch_key(0), ppo.minibatch_counter(u, e)))
    seen.append(ppo.batch_permutation(n, ppo.minibatch_key(1), ppo.minibatch_counter(0, 0)))
    seen.append(ppo.batch_permutation(n, ppo.minibatch_key(0, rank=1), ppo.minibatch_counter(0, 0)))
    for i in range(len(seen)):
        for j in range(i):
            assert float((seen[i] == seen[j]).float().mean()) < 0.02, (i, j)   # (a uniform pair agrees at ~1 / n of the places)
    assert len({ppo.minibatch_counter(u, e) for u in range(50) for e in range(50)}) == 2500


def _blocks_per_slice(perm):
    """for n = 65536: how many of the 64 contiguous 1024-blocks of the source each of the 64 slices of 1024 draws from (the minimum)"""
    blk = np.asarray(perm).reshape(64, 1024) // 1024
    return min(len(set(row.tolist())) for row in blk)


def test_slices_mix_the_whole_batch():
    """A condition, not a measurement: every slice of 1024 holds source indices from at least 60 of the 64 contiguous 1024-blocks.  A
    uniform permutation misses a given block in a given slice with probability ~1e-7, so numpy's meets it -- checked here as well."""
    n = 65536
    assert _blocks_per_slice(np.random.default_rng(0).permutation(n)) >= 60
    for key, counter in ((0, 0), (0, 1), (ppo.minibatch_key(3), ppo.minibatch_counter(2, 7)), (1 << 40, 1 << 33)):
        assert _blocks_per_slice(ppo.batch_permutation(n, key, counter).numpy()) >= 60, (key, counter)


# ------------------------------------------------------------------------------------------------ the PyTorch path against a hand loop
def _nets(seed=0):
    torch.manual_seed(seed)
    return nets.make_policy("mlp64x2")


def _batch(actor, n, seed=12, D=16):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, D), generator=g)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    rtg = torch.randn(n, generator=g) * 3
    var = torch.tensor(0.6)
    with torch.no_grad():
        logp = ppo.gaussian_log_prob(actor(obs), acts, var)
    return obs, acts, logp, rtg, var


def _slices(n, size, mode, key, update, ep):
    """the index tensors of epoch `ep`'s slices: what PPOConfig.minibatch_shuffle says, written out"""
    if mode == "none":
        order = torch.arange(n)
    else:
        order = ppo.batch_permutation(n, key, ppo.minibatch_counter(update, ep if mode == "epoch" else 0))
    return [order[lo:lo + size] for lo in range(0, n, size)]


def _hand_loop(batches, n_ep, size, mode, max_norm=None, limit=None, seed=0, stop_after=None):
    """The minibatch update written out for `len(batches)` ranks played by ONE process (1: the single-process update): per step every
    rank's slice by index_select, the gradients averaged, one Adam step of the flat parameters.  Advantages are normalised once, over
    all ranks' samples, from the summed (sum, sum of squares, count).  Returns (flat, loss_history of rank 0, steps taken, per-step kl)."""
    a, c = _nets(seed)
    fp = ppo.FlatParams([a, c], CPU)
    opt = torch.optim.Adam([fp.proxy], lr=LR)
    world, n = len(batches), batches[0][0].shape[0]
    with torch.no_grad():
        raw = [b[3] - c(b[0]).squeeze(-1) for b in batches]
        m = sum(torch.stack([r.double().sum(), (r.double() ** 2).sum(), torch.tensor(float(r.numel()), dtype=torch.float64)]) for r in raw)
        mean = m[0] / m[2]
        std = torch.sqrt(torch.clamp((m[1] - m[2] * mean * mean) / (m[2] - 1), min=0.0))
        advs = [(r - mean.float()) / (std.float() + 1e-10) for r in raw]
    n_a = fp.module_numel[0]
    K = -(-n // size)
    rows, kls, steps = [], [], 0
    for ep in range(n_ep):
        idx = [_slices(n, size, mode, ppo.minibatch_key(0, r), 0, ep) for r in range(world)]
        for j in range(K):
            grads, kl = [], torch.zeros(2)
            for r, (obs, acts, logp_old, rtg, var) in enumerate(batches):
                i = idx[r][j]
                al, cl, ratios, logp, _ = ppo.ppo_losses(a, c, obs.index_select(0, i), acts.index_select(0, i), logp_old.index_select(0, i),
                                                         rtg.index_select(0, i), advs[r].index_select(0, i), var, CLIP)
                fp.grad.zero_()
                (al + cl).backward()
                grads.append(fp.grad.clone())
                lr_ = logp.detach() - logp_old.index_select(0, i)
                kl += torch.stack([((ratios.detach() - 1) - lr_).sum(), torch.tensor(float(i.numel()))])
                if r == 0:
                    row = torch.stack([al.detach(), cl.detach()])
            rows.append(row)
            kls.append(float(kl[0] / kl[1]))
            if (limit is not None and not (kls[-1] <= limit)) or steps == stop_after:
                hist = _epoch_means(rows, K, n_ep)
                return fp.flat.detach().clone(), hist, steps, kls
            with torch.no_grad():
                fp.grad.copy_(sum(grads))
                if world > 1:
                    fp.grad.div_(world)
                if max_norm is not None:
                    for g in (fp.grad[:n_a], fp.grad[n_a:]):
                        g.mul_(torch.clamp(max_norm / ((g * g).sum().sqrt() + 1e-6), max=1.0))
            opt.step()
            steps += 1
    return fp.flat.detach().clone(), _epoch_means(rows, K, n_ep), steps, kls


def _epoch_means(rows, K, n_ep):
    """row e: the mean over the steps of epoch e that ran, NaN where none did"""
    out = torch.full((n_ep, 2), math.nan)
    for e in range(n_ep):
        mine = rows[e * K:(e + 1) * K]
        if mine:
            out[e] = torch.stack(mine).sum(0) / len(mine)
    return out


def _same_history(got, want):
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


@pytest.mark.parametrize("mode", ["epoch", "update", "none"])
@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_pytorch_path_equals_a_hand_written_loop_over_slices(mode, max_grad_norm):
    n, size, n_ep = 3 * 96 + 40, 96, 3
    a, c = _nets()
    b = _batch(a, n)
    want, hist, steps, _ = _hand_loop([b], n_ep, size, mode, max_norm=max_grad_norm)
    assert steps == n_ep * 4
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, minibatch_size=size, minibatch_shuffle=mode,
                                            max_grad_norm=max_grad_norm), None, CPU)
    st = up.update(*b)
    assert torch.equal(up.fp.flat, want)
    _same_history(up.loss_history, hist)
    assert up.opt.state[up.fp.proxy]["step"] == steps and "kl_stop_step" not in st
    if max_grad_norm is not None:
        assert up.clip_stats.shape == (steps, 4) and bool((up.clip_stats[:, 2:] > 0).all())
    if mode != "none":   # the shuffle is not the identity: the slices differ from the time slices
        un, _, _, _ = _hand_loop([b], n_ep, size, "none", max_norm=max_grad_norm)
        assert not torch.equal(want, un)


def test_an_early_stop_in_the_middle_of_an_epoch():
    n, size, n_ep, K = 3 * 96 + 40, 96, 3, 4
    a, c = _nets()
    b = _batch(a, n)
    _, _, _, kls = _hand_loop([b], n_ep, size, "epoch")
    # a limit between the largest approx_kl of the first 5 steps and that of step 6 (0-based 5: the second slice of the second epoch)
    trip = next(k for k in range(5, len(kls)) if kls[k] > max(kls[:k]))
    assert trip % K != 0, kls
    limit = 0.5 * (max(kls[:trip]) + kls[trip])
    want, hist, steps, _ = _hand_loop([b], n_ep, size, "epoch", limit=limit)
    assert steps == trip
    before, _, s2, _ = _hand_loop([b], n_ep, size, "epoch", stop_after=trip)
    assert s2 == trip and torch.equal(before, want)   # the parameters before the tripping step
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, minibatch_size=size, target_kl=limit / 1.5),
                        None, CPU)
    st = up.update(*b)
    assert st["kl_stop_step"] == trip and st["kl_stop_epoch"] == trip // K and st["kl_stopped"] == 1
    assert torch.equal(up.fp.flat, want)
    _same_history(up.loss_history, hist)
    assert bool(torch.isnan(up.loss_history[trip // K + 1:]).all()) and bool(torch.isfinite(up.loss_history[:trip // K + 1]).all())
    assert up.opt.state[up.fp.proxy]["step"] == trip
    assert torch.equal(up.clip_stats[trip, 2:], torch.zeros(2)) and bool((up.clip_stats[:trip, 2:] == 1).all())


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad", [0, -32, 31, 33, 100, 48, 32.0, True])
def test_minibatch_size_must_be_a_positive_multiple_of_32(bad):
    with pytest.raises(ValueError):
        ppo.PPOConfig(minibatch_size=bad)
    cfg = ppo.PPOConfig(policy="mlp64x2")
    cfg.minibatch_size = bad   # (a config is mutable: the updater checks again)
    with pytest.raises(ValueError):
        ppo.PPOUpdater(*_nets(), cfg, None, CPU)


def test_shuffle_mode_overlap_and_defaults():
    cfg = ppo.PPOConfig()
    assert cfg.minibatch_size is None and cfg.minibatch_shuffle == "epoch"
    assert ppo.PPOConfig(minibatch_size=64, minibatch_shuffle="update").minibatch_size == 64
    with pytest.raises(ValueError):
        ppo.PPOConfig(minibatch_shuffle="batch")
    with pytest.raises(ValueError):
        ppo.PPOConfig(minibatch_size=64, overlap_allreduce=True)
    assert ppo.PPOConfig(overlap_allreduce=True).minibatch_size is None


def test_cli_flags_reach_the_config():
    args = cli.get_args(["--minibatch_size", "256", "--minibatch_shuffle", "update", "--policy", "mlp64x2"])
    cfg = cli.config_of(args, 16)
    assert cfg.minibatch_size == 256 and cfg.minibatch_shuffle == "update" and cfg.rollout_len == 16
    cfg = cli.config_of(cli.get_args([]), 8)
    assert cfg.minibatch_size is None and cfg.minibatch_shuffle == "epoch"
    with pytest.raises(SystemExit):
        cli.get_args(["--minibatch_shuffle", "sometimes"])


# ------------------------------------------------------------------------------------------------ the full batch is what it was
@pytest.mark.parametrize("extra", [{}, {"max_grad_norm": 0.5}, {"target_kl": 1e6}])
def test_none_and_a_size_at_or_above_the_batch_are_the_full_batch_update(extra):
    n = 200
    res = []
    for mb in (None, 224, 4096):   # (224 >= 200: the smallest multiple of 32 at or above the batch)
        a, c = _nets()
        b = _batch(a, n)
        up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=3, minibatch_size=mb, **extra), None, CPU)
        st = up.update(*b)
        res.append((up.fp.flat.clone(), st, up.loss_history.clone()))
    want, _, _, _ = _hand_loop([_batch(_nets()[0], n)], 3, n, "none", max_norm=extra.get("max_grad_norm"))
    assert torch.equal(res[0][0], want)   # ... and that is the whole-batch loop, one step per epoch
    for flat, st, hist in res[1:]:
        assert torch.equal(flat, res[0][0]) and torch.equal(hist, res[0][2])
        assert st == res[0][1] and list(st) == list(res[0][1]) and "kl_stop_step" not in st


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _rank_batch(rank, n):
    return _batch(_nets()[0], n, seed=40 + rank)


def _mb_worker(rank, world, port, path, ns, n_ep, size):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    ctx = ppo.DistCtx(device="cpu")
    a, c = _nets()
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, minibatch_size=size), ctx, CPU)
    out = {}
    try:
        up.update(*_rank_batch(rank, ns[rank]))
        out = {"flat": up.fp.flat.clone(), "hist": up.loss_history.clone(), "t": int(up.opt.state[up.fp.proxy]["step"])}
    except ValueError as e:
        out = {"error": str(e)}
    torch.save(out, f"{path}.{rank}")
    ctx.barrier()
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_equal_one_process_that_plays_both(tmp_path):
    from _ranks import spawn_ranks
    n, size, n_ep = 2 * 64 + 24, 64, 2
    path = str(tmp_path / "mb")
    spawn_ranks(_mb_worker, 2, lambda port: (2, port, path, (n, n), n_ep, size))
    r0, r1 = (torch.load(f"{path}.{k}") for k in range(2))
    assert torch.equal(r0["flat"], r1["flat"]) and r0["t"] == r1["t"] == n_ep * 3
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (as the ranks ran)
    try:
        want, hist, steps, _ = _hand_loop([_rank_batch(0, n), _rank_batch(1, n)], n_ep, size, "epoch")
    finally:
        torch.set_num_threads(threads)
    assert steps == n_ep * 3 and torch.equal(r0["flat"], want)
    _same_history(r0["hist"], hist)


def test_unequal_batches_across_ranks_raise_on_every_rank(tmp_path):
    from _ranks import spawn_ranks
    path = str(tmp_path / "mbne")
    spawn_ranks(_mb_worker, 2, lambda port: (2, port, path, (160, 128), 1, 64))
    for k in range(2):
        r = torch.load(f"{path}.{k}")
        assert "same number of samples" in r.get("error", ""), r
