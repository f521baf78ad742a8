"""The KL-adaptive learning rate of the fused PPO update (navppo_*_update_epoch_lr, navppo_adam_step_lr, PPOConfig.lr_schedule =
"adaptive") on the GPU, for every family of fused kernels (the shapes of tests/test_gpu_grad_clip.py).

The new code is the step launch: it derives the step's rate from the rate slot the call before wrote and from approx_kl, then runs the
clipped epoch's step.  So every check here is exact: an *_lr call equals the *_clipped call whose `lr` argument is the host mirror's
(ppo.adaptive_lr_reference) value, bit for bit; only navppo_adam_step_lr is also held against float64 Adam (the bounds of _check_adam)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from navbot_ppo_amd import ppo
from navbot_ppo_amd._native import lib
from test_gpu_grad_clip import DEV, FAMILIES, HYPER, INF, P, _check_adam, _ok, _same, _st, fam_ids
from test_gpu_target_kl import KLFamily

pytestmark = pytest.mark.gpu
f32 = np.float32
LR0 = float(f32(3e-4))
LR_UP2 = float(f32(3e-4) * f32(1.5) * f32(1.5))      # two raises from LR0, as the kernel computes them
LR_DOWN2 = float(f32(3e-4) / f32(1.5) / f32(1.5))    # two lowerings
BETAS = HYPER[1:]
KEYS = ("p", "m", "v", "g")


class LrFamily(KLFamily):
    def start(self, used=False):
        s = super().start(used)
        s.update(lr=torch.zeros(4, device=DEV))
        return s

    def _epoch(self, name, s, step, lr, tail, logp=None, st=None):
        _ok(getattr(self.L, name)(P(s["p"]), *self._oargs(self.obs), P(self.acts), P(self.logp if logp is None else logp), P(self.rtg),
                                  P(self.adv), self.n, 0.6, 0.2, lr, *BETAS, step, P(s["m"]), P(s["v"]), P(s["g"]),
                                  P(s["st"]) if st is None else st, P(self.ws), *tail, _st()), name)

    def epoch_lr(self, s, step, kl_target, adapt, max_norm=INF, lr=LR0, lr_min=1e-5, lr_max=1e-2, logp=None, st=None, sync=True):
        """one *_update_epoch_lr call in place on state s (clip_stats in s["cs"], the rate state in s["lr"])"""
        self._epoch(self.prefix + "update_epoch_lr", s, step, lr, (max_norm, P(s["cs"]), kl_target, lr_min, lr_max, adapt, P(s["lr"])), logp, st)
        if sync:
            torch.cuda.synchronize()

    def epoch_clipped(self, s, step, lr, max_norm=INF, logp=None):
        """one *_update_epoch_clipped call with an explicit learning rate"""
        self._epoch(self.prefix + "update_epoch_clipped", s, step, lr, (max_norm, P(s["cs"])), logp)
        torch.cuda.synchronize()


_fams = {}


def _family(kind, D, f16, n):
    """the family and its pilot run, computed once and left unchanged: the approx_kl of eight *_clipped(max_norm = +inf) epochs at LR0"""
    key = (kind, D, f16, n)
    if key not in _fams:
        fam = LrFamily(kind, D, f16, n)
        s, kls = fam.start(), []
        for step in range(1, 9):
            fam.epoch_clipped(s, step, LR0)
            kls.append(float(s["st"][1]))
        _fams[key] = (fam, kls)
    return _fams[key]


def _queued_run(fam, kl_target, lr_min, lr_max, n_calls=8, step0=1, max_norm=INF):
    """Run A: n_calls *_lr calls queued with NO synchronisation between them, adapt = 0, 1, 1, ...; every call's statistics in a row of
    its own, the state after every call copied on the stream.  Returns (snapshots, kl per call, rate state after every call)."""
    s = fam.start()
    stats = torch.zeros((n_calls, 8), device=DEV)
    snaps, states = [], []
    for k in range(n_calls):
        fam.epoch_lr(s, step0 + k, kl_target, int(k > 0), max_norm, lr_min=lr_min, lr_max=lr_max,
                     st=C.c_void_p(stats.data_ptr() + 32 * k), sync=False)
        snaps.append({key: s[key].clone() for key in KEYS + ("cs",)})
        states.append(s["lr"].clone())
    torch.cuda.synchronize()
    return snaps, stats[:, 1].cpu(), [t.tolist() for t in states]


def _replay(fam, kls, snaps, states, kl_target, lr_min, lr_max, step0=1, max_norm=INF):
    """Run B: from the same start, *_clipped calls whose lr is the mirror's, fed A's recorded kl; everything equal after every step."""
    b = fam.start()
    lr, ups, downs, dirs = LR0, 0, 0, []
    for k, kl in enumerate(kls.tolist()):
        d = ppo.adaptive_lr_direction(kl, kl_target, adapt=k > 0)
        lr = ppo.adaptive_lr_reference(lr, kl, kl_target, lr_min, lr_max, adapt=k > 0)
        ups, downs = ups + (d > 0), downs + (d < 0)
        dirs.append(d)
        fam.epoch_clipped(b, step0 + k, lr, max_norm)
        assert all(torch.equal(snaps[k][key], b[key]) for key in KEYS), (k, lr)
        assert torch.equal(snaps[k]["cs"], b["cs"]), k
        kb = float(b["st"][1])
        assert kb == kl or (math.isnan(kb) and math.isnan(kl)), (k, kb, kl)
        st = states[k]
        assert st[(step0 + k + 1) & 1] == lr and st[2] == float(ups) and st[3] == float(downs), (k, st, lr, ups, downs)
    return dirs, lr


@pytest.mark.parametrize("max_norm", [INF, 0.05])
@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_adapt_off_is_the_clipped_epoch(kind, D, f16, n, max_norm):
    fam, _ = _family(kind, D, f16, n)
    a, b = fam.start(), fam.start()
    for step in range(1, 6):
        fam.epoch_lr(a, step, 0.01, 0, max_norm)
        cs = fam.epoch(b, step, max_norm)
        assert _same(a, b), step
        assert torch.equal(a["st"][[0, 1, 2, 4]], b["st"][[0, 1, 2, 4]]) and torch.equal(a["cs"], cs), step
    assert a["lr"].tolist() == [LR0, LR0, 0.0, 0.0]
    assert not torch.equal(a["p"], fam.flat)


@pytest.mark.parametrize("target", ["raise", "lower", "pilot"])
@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_queued_run_is_the_host_stepped_replay(kind, D, f16, n, target):
    fam, pilot = _family(kind, D, f16, n)
    if target == "raise":     # every adapting step raises, until lr_max = LR0 x 1.5^2 holds the rate
        kl_target, lr_min, lr_max = 1e3, 1e-5, LR_UP2
    elif target == "lower":   # every adapting step lowers, until lr_min = LR0 / 1.5^2 holds the rate
        kl_target, lr_min, lr_max = 1e-30, LR_DOWN2, 1e-2
    else:
        lr_min, lr_max = 1e-5, 1e-2
    if target != "pilot":
        snaps, kls, states = _queued_run(fam, kl_target, lr_min, lr_max)
    else:
        # a target from the pilot's own values (kl starts at 0): a multiple of one of the early calls', the first one under which the
        # eight steps raise, hold and lower.  (The 2x64 heads' kl grows steadily at LR0 and 4 x the fourth call's does it; the 512-wide
        # nets overshoot and come back, so more candidates are tried -- a run costs eight epochs.)
        assert min(pilot[1:4]) > 0, pilot
        for base, mult in [(j, m) for j in (3, 1, 2) for m in (4.0, 2.0, 8.0, 1.0, 16.0, 3.0, 1.5, 0.5)]:
            kl_target = float(f32(mult * pilot[base]))
            snaps, kls, states = _queued_run(fam, kl_target, lr_min, lr_max)
            seen = {ppo.adaptive_lr_direction(kl, kl_target, adapt=k > 0) for k, kl in enumerate(kls.tolist())}
            print(f"{kind} d{D} n{n}: target {mult} x pilot kl[{base}] = {kl_target:.3e}: kl {kls.tolist()} -> directions {sorted(seen)}")
            if seen == {-1, 0, 1}:
                break
    dirs, lr = _replay(fam, kls, snaps, states, kl_target, lr_min, lr_max)
    print(f"{kind} d{D} n{n} {target}: directions {dirs}, final lr {lr:.6e}")
    if target == "raise":
        # (call k has step k + 1 and writes slot k & 1)
        assert dirs == [0] + [1] * 7 and lr == LR_UP2 and states[2][0] == LR_UP2 and states[1][1] == float(f32(3e-4) * f32(1.5))
    elif target == "lower":
        assert dirs == [0] + [-1] * 7 and lr == LR_DOWN2 and states[2][0] == LR_DOWN2
    else:
        assert dirs[0] == 0 and set(dirs) == {-1, 0, 1}, dirs


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_nan_kl_lowers_once_and_the_guard_is_the_clipped_epochs(kind, D, f16, n):
    fam, _ = _family(kind, D, f16, n)
    logp = fam.logp.clone()
    logp[n // 3] = float("nan")
    a, b = fam.start(used=True), fam.start(used=True)
    fam.epoch_lr(a, 2, 0.01, 1, 0.05, logp=logp)   # (step 2: reads slot 0, writes slot 1)
    lr = ppo.adaptive_lr_reference(LR0, float("nan"), 0.01, 1e-5, 1e-2)
    assert lr == float(f32(3e-4) / f32(1.5))
    fam.epoch_clipped(b, 2, lr, 0.05, logp=logp)
    assert math.isnan(float(a["st"][1]))
    assert a["lr"].tolist() == [0.0, lr, 0.0, 1.0]
    for k in KEYS:   # (bit patterns: the actor's gradient holds NaNs)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(a["cs"][2:], b["cs"][2:]) and float(a["cs"][2]) == 0.0 and not math.isfinite(float(a["cs"][0]))
    assert float(a["cs"][3]) > 0.0 and float(a["cs"][1]) == float(b["cs"][1])
    PA = fam.PA   # the actor (squared norm not finite) keeps parameters and moments; the critic stepped, with the lowered rate
    for k, t0 in (("p", fam.flat), ("m", fam.m0), ("v", fam.v0)):
        assert torch.equal(a[k][:PA], t0[:PA]) and not torch.equal(a[k][PA:], t0[PA:]), k


@pytest.mark.parametrize("kind,D,f16,n", [FAMILIES[0], FAMILIES[5], FAMILIES[6]], ids=[fam_ids[0], fam_ids[5], fam_ids[6]])
def test_slots(kind, D, f16, n):
    fam, _ = _family(kind, D, f16, n)
    pre = float(f32(1e-3))
    # both slots preset: the lr argument is ignored
    a, b = fam.start(), fam.start()
    a["lr"][:2] = pre
    for step in (1, 2):
        fam.epoch_lr(a, step, 0.01, 0, lr=LR0)
        fam.epoch_clipped(b, step, pre)
        assert _same(a, b), step
    assert a["lr"].tolist() == [pre, pre, 0.0, 0.0]
    # zeroed between two updates: restarts at the argument
    a["lr"].zero_()
    fam.epoch_lr(a, 3, 0.01, 0, lr=LR0)
    fam.epoch_clipped(b, 3, LR0)
    assert _same(a, b) and a["lr"].tolist() == [LR0, 0.0, 0.0, 0.0]
    # an odd and an even first step: the same rates, each run its own clipped replay
    outs = []
    for step0 in (1, 2):
        snaps, kls, states = _queued_run(fam, 1e3, 1e-5, LR_UP2, n_calls=4, step0=step0)
        dirs, _ = _replay(fam, kls, snaps, states, 1e3, 1e-5, LR_UP2, step0=step0)
        assert dirs == [0, 1, 1, 1]
        outs.append([st[(step0 + k + 1) & 1] for k, st in enumerate(states)] + states[-1][2:])
    assert outs[0] == outs[1] == [LR0, float(f32(3e-4) * f32(1.5)), LR_UP2, LR_UP2, 3.0, 0.0]


@pytest.mark.parametrize("kind,D,f16", [("mlp64", 16, 0), ("x3", 42, 0), ("resmlp", 16, 0)])
def test_lr_entry_points_check_their_arguments(kind, D, f16):
    fam = LrFamily(kind, D, f16, 256)
    s = fam.start(used=True)
    s["lr"][:] = torch.tensor([1e-3, 2e-3, 3.0, 4.0])
    L = lib()
    name = fam.prefix + "update_epoch_lr"
    nan = float("nan")

    def call(kl_target=0.01, lr_min=1e-5, lr_max=1e-2, adapt=1, state=s["lr"], max_norm=INF, cs=s["cs"], step=1):
        return getattr(L, name)(P(s["p"]), *fam._oargs(fam.obs), P(fam.acts), P(fam.logp), P(fam.rtg), P(fam.adv), fam.n, 0.6, 0.2, *HYPER, step,
                                P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(fam.ws), max_norm, P(cs), kl_target, lr_min, lr_max, adapt,
                                P(state), _st())
    bad = [dict(kl_target=0.0), dict(kl_target=-1.0), dict(kl_target=nan), dict(lr_min=0.0), dict(lr_min=-1e-5), dict(lr_min=nan),
           dict(lr_max=1e-6), dict(lr_max=nan), dict(adapt=2), dict(adapt=-1), dict(state=None),
           dict(max_norm=0.0), dict(max_norm=nan), dict(cs=None), dict(step=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.navppo_last_error().decode().startswith(name + ": "), (kw, L.navppo_last_error())
    torch.cuda.synchronize()
    assert torch.equal(s["p"], fam.flat) and torch.equal(s["m"], fam.m0) and torch.equal(s["v"], fam.v0)
    assert torch.equal(s["lr"].cpu(), torch.tensor([1e-3, 2e-3, 3.0, 4.0]))
    assert call(lr_min=1e-3, lr_max=1e-3, adapt=0) == 0   # (lr_max == lr_min is allowed)
    torch.cuda.synchronize()
    assert not torch.equal(s["p"], fam.flat)
    t, cs = torch.zeros(64, device=DEV), torch.zeros(4, device=DEV)
    step_lr = lambda kl_target=0.01, lr_min=1e-5, lr_max=1e-2, adapt=1, state=cs, kl=cs, max_norm=INF, stats=cs: L.navppo_adam_step_lr(
        P(t), P(t), P(t), P(t), 64, 32, 0.5, max_norm, *HYPER, 1, P(stats), kl_target, lr_min, lr_max, adapt, P(state), P(kl), _st())
    for kw in bad[:11] + [dict(kl=None), dict(max_norm=0.0), dict(stats=None)]:
        assert step_lr(**kw) == -1, kw
        assert L.navppo_last_error().decode().startswith("navppo_adam_step_lr: "), (kw, L.navppo_last_error())
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(cs.any())


@pytest.mark.parametrize("n,n_first", [(5378 + 5313, 5378), (257, 100), (5313, 0)])
def test_adam_step_lr(n, n_first):
    """The multi-GPU form with kl_dev set to force each outcome: the step against float64 Adam at the mirror's rate (and bit-equal to
    navppo_adam_step_clipped at that rate), grad_dev = grad x grad_scale x coef, the state as in the queued run."""
    L = lib()
    gen = torch.Generator().manual_seed(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.05
    m0, v0 = torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-6
    tgt = 0.01
    for (kl, want_dir), (max_norm, step) in zip(((0.021, -1), (0.01, 0), (0.004, 1), (float("nan"), -1)), ((INF, 1), (0.1, 5), (0.1, 2), (INF, 4))):
        klv = torch.tensor([kl], device=DEV)
        lr = ppo.adaptive_lr_reference(LR0, kl, tgt, 1e-5, 1e-2)
        assert ppo.adaptive_lr_direction(kl, tgt) == want_dir and (lr != LR0) == (want_dir != 0)
        p, g, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        pc, gc, mc, vc = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        cs, csc, state = torch.full((4,), -7.0, device=DEV), torch.full((4,), -7.0, device=DEV), torch.zeros(4, device=DEV)
        _ok(L.navppo_adam_step_lr(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step, P(cs), tgt, 1e-5, 1e-2, 1, P(state), P(klv),
                                  _st()), "adam_step_lr")
        _ok(L.navppo_adam_step_clipped(P(pc), P(gc), P(mc), P(vc), n, n_first, 0.5, max_norm, lr, *BETAS, step, P(csc), _st()), "clipped")
        torch.cuda.synchronize()
        want = [0.0, 0.0, float(want_dir > 0), float(want_dir < 0)]
        want[(step + 1) & 1] = lr
        assert state.tolist() == want, (state, want)
        for x, y in ((p, pc), (g, gc), (m, mc), (v, vc), (cs, csc)):
            assert torch.equal(x, y)
        _check_adam(p0, m0, v0, g, step, p, m, v, lr=lr, what=f"adam_step_lr n={n} n_first={n_first} step={step} kl={kl}")
        c = cs.double().cpu()
        for k, sl in enumerate((slice(0, n_first), slice(n_first, n))):
            exp = g0.double()[sl] * 0.5 * float(c[2 + k])
            assert bool(((g.double().cpu()[sl] - exp).abs() <= 2 * 2.0 ** -23 * exp.abs() + 2.0 ** -140).all()), k
        # adapt = 0 on the state this call left: the rate stays, the counts stay
        _ok(L.navppo_adam_step_lr(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step + 1, P(cs), tgt, 1e-5, 1e-2, 0, P(state), P(klv),
                                  _st()), "adam_step_lr")
        torch.cuda.synchronize()
        assert state.tolist() == [lr, lr] + want[2:]


def _replay_log(kls, lr, cfg):
    ups = downs = 0
    for k, kl in enumerate(kls):
        d = ppo.adaptive_lr_direction(kl, cfg.desired_kl, adapt=k > 0)
        lr = ppo.adaptive_lr_reference(lr, kl, cfg.desired_kl, cfg.lr_min, cfg.lr_max, adapt=k > 0)
        ups, downs = ups + (d > 0), downs + (d < 0)
    return lr, ups, downs


def _trainer(policy, iters=2, **kw):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(64, map="stage_1", max_episode_steps=20, seed=1)
    cfg = ppo.PPOConfig(rollout_len=32, max_episode_steps=20, n_updates_per_iteration=6, policy=policy, seed=2, **kw)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.updater.fused
    logs, kls = [], []
    for _ in range(iters):
        logs.append(dict(tr.iteration()))
        kls.append(None if tr.updater.kl_steps is None else tr.updater.kl_steps.tolist())
    torch.cuda.synchronize()
    out = dict(flat=tr.updater.fp.flat.clone(), m=tr.updater._adam_m.clone(), v=tr.updater._adam_v.clone(), logs=logs, kls=kls, cfg=cfg,
               tb=tr.tb_scalars(), state=None if tr.updater.lr_state is None else tr.updater.lr_state.tolist(), t=tr.updater._adam_t)
    env.close()
    return out


@pytest.mark.parametrize("minibatch_size", [None, 512])
@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_logs_what_the_mirror_replays(policy, minibatch_size):
    A = _trainer(policy, lr_schedule="adaptive", minibatch_size=minibatch_size)
    n_st = 6 * (4 if minibatch_size else 1)
    lr, changes = A["cfg"].lr, 0
    for lg, kls in zip(A["logs"], A["kls"]):
        assert len(kls) == n_st
        lr, ups, downs = _replay_log(kls, lr, A["cfg"])   # (the second iteration starts at the first one's final rate)
        print(f"{policy} mb {minibatch_size}: kl {kls} -> lr {lr:.6e} ups {ups} downs {downs}; logged {lg['lr']:.6e} {lg['lr_ups']} {lg['lr_downs']}")
        assert (lg["lr"], lg["lr_ups"], lg["lr_downs"]) == (lr, ups, downs)
        changes += ups + downs
    assert changes > 0 and A["t"] == 2 * n_st
    assert A["state"][(A["t"] + 1) & 1] == lr and A["tb"]["ppo/lr"] == lr and A["tb"]["ppo/lr_ups"] == A["logs"][-1]["lr_ups"]
    # lr_schedule=None beside it: the path of before (no lr keys), and the weights of an adaptive run whose clamps pin the rate at cfg.lr
    # -- *_lr at a constant rate and max_norm = +inf has the bits of the plain epoch
    N = _trainer(policy, minibatch_size=minibatch_size)
    assert "lr" not in N["logs"][0] and "ppo/lr" not in N["tb"] and N["state"] is None and N["kls"] == [None, None]
    Pn = _trainer(policy, lr_schedule="adaptive", lr_min=3e-4, lr_max=3e-4, minibatch_size=minibatch_size)
    for k in ("flat", "m", "v"):
        assert torch.equal(N[k], Pn[k]), k
    assert not torch.equal(N["flat"], A["flat"])
    assert Pn["logs"][-1]["lr"] == LR0


def _dp_lr_worker(rank, world, port, path, policy):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduces here
    from navbot_ppo_amd import ppo
    from navbot_ppo_amd.env import VecEnv
    ctx = ppo.DistCtx(device="cuda:0")
    lo, hi = ctx.shard(128)
    env = VecEnv(hi - lo, map="stage_1", max_episode_steps=20, seed=3, env_id_base=lo, device="cuda:0")
    cfg = ppo.PPOConfig(rollout_len=32, max_episode_steps=20, n_updates_per_iteration=5, policy=policy, seed=5, lr_schedule="adaptive")
    tr = ppo.PPOTrainer(env, cfg, ctx)
    lgs, kls = [], []
    for _ in range(2):
        lg = tr.iteration()
        lgs.append({k: lg[k] for k in ("lr", "lr_ups", "lr_downs", "approx_kl")})
        kls.append(tr.updater.kl_steps.tolist())
    torch.cuda.synchronize()
    torch.save({"flat": tr.updater.fp.flat.cpu(), "m": tr.updater._adam_m.cpu(), "v": tr.updater._adam_v.cpu(),
                "state": tr.updater.lr_state.cpu(), "kls": kls, "logs": lgs}, f"{path}.{rank}")
    ctx.barrier()
    env.close()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_two_ranks_step_with_the_same_rate(tmp_path, policy):
    """Two gloo ranks sharing the GPU: passes -> all-reduce of the gradient and of [kl n, n] -> navppo_adam_step_lr.  The ranks' shards
    differ, the global approx_kl does not: equal rates at every step, equal weights and moments."""
    from _ranks import spawn_ranks
    path = str(tmp_path / "dplr")
    spawn_ranks(_dp_lr_worker, 2, lambda port: (2, port, path, policy))
    r0, r1 = torch.load(path + ".0"), torch.load(path + ".1")
    for k in ("flat", "m", "v", "state"):
        assert torch.equal(r0[k], r1[k]), k
    assert bool(torch.isfinite(r0["flat"]).all()) and r0["kls"] == r1["kls"] and r0["logs"] == r1["logs"]
    cfg, lr, changes = ppo.PPOConfig(lr_schedule="adaptive"), 3e-4, 0
    for lg, kls in zip(r0["logs"], r0["kls"]):   # the rate of every step, from the mirror over the global kl both ranks recorded
        lr, ups, downs = _replay_log(kls, lr, cfg)
        assert (lg["lr"], lg["lr_ups"], lg["lr_downs"]) == (lr, ups, downs)
        changes += ups + downs
    assert changes >= 1 and float(r0["state"][(10 + 1) & 1]) == lr
