"""The early stop of the fused PPO update at a KL limit (navppo_*_update_epoch_kl, navppo_adam_step_kl, PPOConfig.target_kl) on the
GPU, for every family of fused kernels (the shapes of tests/test_gpu_grad_clip.py).

The batches' logp_old is the START policy's own log-probability of the batch actions, so approx_kl starts at 0 and grows as the weights
move.  Before a trip the gated epochs are bit-identical to the clipped ones, so the device's own approx_kl values decide where the stop
falls: no tolerance is involved anywhere but in the float64 checks of navppo_adam_step_kl."""
import ctypes as C
import math
import os

import pytest
import torch

from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd._native import lib
from test_gpu_grad_clip import DEV, FAMILIES, HYPER, INF, Family, P, _check_adam, _ok, _same, _st, fam_ids

pytestmark = pytest.mark.gpu


class KLFamily(Family):
    def __init__(self, kind, D, f16, n, seed=11):
        super().__init__(kind, D, f16, n, seed)
        torch.manual_seed(seed)   # the start weights of Family: the same nets again
        a, _ = nets.make_policy("resmlp512" if kind == "resmlp" else "mlp64x2", **({} if kind == "resmlp" else dict(obs_dim=D)))
        with torch.no_grad():
            self.logp = ppo.gaussian_log_prob(a(self.obs.float().cpu()), self.acts.cpu(), torch.tensor(0.6)).to(DEV).contiguous()

    def start(self, used=False):
        s = super().start(used)
        s.update(cs=torch.full((4,), -7.0, device=DEV), kl=torch.zeros(4, device=DEV))
        return s

    def epoch_kl(self, s, step, kl_limit, max_norm=INF, logp=None):
        """one *_update_epoch_kl call in place on state s (clip_stats in s["cs"], the KL state in s["kl"])"""
        name = self.prefix + "update_epoch_kl"
        _ok(getattr(self.L, name)(P(s["p"]), *self._oargs(self.obs), P(self.acts), P(self.logp if logp is None else logp), P(self.rtg),
                                  P(self.adv), self.n, 0.6, 0.2, *HYPER, step, P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(self.ws),
                                  max_norm, P(s["cs"]), kl_limit, P(s["kl"]), _st()), name)
        torch.cuda.synchronize()


_fams = {}


def _family(kind, D, f16, n):
    """the family and its reference run, computed once and left unchanged: six *_clipped(max_norm = +inf) epochs, the state after each"""
    key = (kind, D, f16, n)
    if key not in _fams:
        fam = KLFamily(kind, D, f16, n)
        s, ref = fam.start(), []
        for step in range(1, 7):
            cs = fam.epoch(s, step, INF)
            ref.append(dict({k: s[k].clone() for k in ("p", "m", "v", "g", "st")}, cs=cs.clone(), kl=float(s["st"][1])))
        _fams[key] = (fam, ref)
    return _fams[key]


@pytest.mark.parametrize("max_norm", [INF, 0.05])
@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_infinite_limit_is_the_clipped_epoch(kind, D, f16, n, max_norm):
    fam, _ = _family(kind, D, f16, n)
    a, b = fam.start(), fam.start()
    for step in range(1, 6):
        fam.epoch_kl(a, step, INF, max_norm)
        cs = fam.epoch(b, step, max_norm)
        assert _same(a, b), step
        assert torch.equal(a["st"][[0, 1, 2, 4]], b["st"][[0, 1, 2, 4]]) and torch.equal(a["cs"], cs), step
    assert a["kl"].tolist() == [0.0, 5.0, 0.0, 0.0]
    assert not torch.equal(a["p"], fam.flat)


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_trips_at_the_first_epoch_over_the_limit_then_is_sticky(kind, D, f16, n):
    fam, ref = _family(kind, D, f16, n)
    j = 3 if kind == "resmlp" else 4
    kls = [r["kl"] for r in ref]
    lo, hi = max(kls[:j - 1]), kls[j - 1]
    print(f"{kind} d{D} n{n}: approx_kl of epochs 1..6 = {kls}; KL_{j} / max(earlier) = {hi / lo if lo > 0 else math.inf:.3f}")
    assert hi >= 1.5 * lo, (kls, j)                    # the precondition: a gap wide enough to put the limit into
    kl_limit = float(torch.tensor(0.5 * (lo + hi), dtype=torch.float32))
    assert lo < kl_limit < hi
    s = fam.start()
    for step in range(1, j):
        fam.epoch_kl(s, step, kl_limit)
        assert _same(s, ref[step - 1]), step
        assert s["kl"].tolist() == [0.0, float(step), 0.0, 0.0]
    fam.epoch_kl(s, j, kl_limit)                       # the trip: nothing is stepped, the pass results are epoch j's
    for k in ("p", "m", "v"):
        assert torch.equal(s[k], ref[j - 2][k]), k
    assert torch.equal(s["g"], ref[j - 1]["g"])       # (max_norm = +inf: the reference's clipped gradient is the unclipped sum)
    assert torch.equal(s["st"][[0, 1, 2, 4]], ref[j - 1]["st"][[0, 1, 2, 4]])
    assert torch.equal(s["cs"][:2], ref[j - 1]["cs"][:2]) and s["cs"][2:].tolist() == [0.0, 0.0]
    assert s["kl"].tolist() == [1.0, float(j - 1), hi, float(j)]
    keep = {k: s[k].clone() for k in ("p", "m", "v", "kl")}
    for step in (j + 1, j + 2):                        # stopped: every kernel returns at its entry
        for k in ("g", "st", "cs"):
            s[k].fill_(-7.0)
        fam.epoch_kl(s, step, kl_limit)
        for k in ("p", "m", "v", "kl"):
            assert torch.equal(s[k], keep[k]), (k, step)
        for k in ("g", "st", "cs"):
            assert bool((s[k] == -7.0).all()), (k, step)
    # a limit above every epoch's value on the same state buffer, zeroed: the update runs again
    s["kl"].zero_()
    fam.epoch_kl(s, j, INF)
    assert s["kl"].tolist() == [0.0, 1.0, 0.0, 0.0] and not torch.equal(s["p"], keep["p"])


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_nan_kl_trips(kind, D, f16, n):
    fam, _ = _family(kind, D, f16, n)
    logp = fam.logp.clone()
    logp[n // 3] = float("nan")
    s = fam.start(used=True)
    fam.epoch_kl(s, 1, 1e30, logp=logp)
    st = s["kl"].tolist()
    assert st[0] == 1.0 and st[1] == 0.0 and math.isnan(st[2]) and st[3] == 1.0
    for k, t0 in (("p", fam.flat), ("m", fam.m0), ("v", fam.v0)):
        assert torch.equal(s[k], t0), k
    assert s["cs"][2:].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("kind,D,f16", [("mlp64", 16, 0), ("x3", 42, 0), ("resmlp", 16, 0)])
def test_kl_entry_points_check_their_arguments(kind, D, f16):
    fam = KLFamily(kind, D, f16, 256)
    s = fam.start()
    L = lib()
    name = fam.prefix + "update_epoch_kl"

    def call(kl_limit, state, max_norm=INF):
        return getattr(L, name)(P(s["p"]), *fam._oargs(fam.obs), P(fam.acts), P(fam.logp), P(fam.rtg), P(fam.adv), fam.n, 0.6, 0.2, *HYPER, 1,
                                P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(fam.ws), max_norm, P(s["cs"]), kl_limit, P(state), _st())
    for bad in (0.0, -1.0, float("nan")):
        assert call(bad, s["kl"]) == -1 and b"kl_limit" in L.navppo_last_error()
    assert call(1.0, None) == -1 and b"kl_state_dev" in L.navppo_last_error()
    assert call(1.0, s["kl"], max_norm=0.0) == -1 and b"max_norm" in L.navppo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(s["p"], fam.flat) and s["kl"].tolist() == [0.0] * 4
    assert call(INF, s["kl"]) == 0
    torch.cuda.synchronize()
    assert s["kl"].tolist() == [0.0, 1.0, 0.0, 0.0] and not torch.equal(s["p"], fam.flat)
    t, cs = torch.zeros(64, device=DEV), torch.zeros(4, device=DEV)
    for bad in (0.0, -1.0, float("nan")):
        assert L.navppo_adam_step_kl(P(t), P(t), P(t), P(t), 64, 32, 0.5, INF, *HYPER, 1, P(cs), bad, P(cs), P(cs), _st()) == -1
    assert L.navppo_adam_step_kl(P(t), P(t), P(t), P(t), 64, 32, 0.5, INF, *HYPER, 1, P(cs), 1.0, None, P(cs), _st()) == -1
    assert L.navppo_adam_step_kl(P(t), P(t), P(t), P(t), 64, 32, 0.5, INF, *HYPER, 1, P(cs), 1.0, P(cs), None, _st()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,n_first", [(5378 + 5313, 5378), (257, 100), (5313, 0)])
def test_adam_step_kl(n, n_first):
    """Below the limit: navppo_adam_step_clipped's result (float64 bounds of _check_adam; bit-equal to the clipped entry point).  Above
    it: parameters, moments and the gradient untouched, clip_stats = (s_actor, s_critic, 0, 0), the state set; then sticky."""
    L = lib()
    gen = torch.Generator().manual_seed(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.05
    m0, v0 = torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-6
    kl = torch.tensor([0.02], device=DEV)
    for max_norm, step in ((INF, 1), (0.1, 5)):
        p, g, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        pc, gc, mc, vc = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        cs, csc, state = torch.full((4,), -7.0, device=DEV), torch.full((4,), -7.0, device=DEV), torch.zeros(4, device=DEV)
        _ok(L.navppo_adam_step_kl(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step, P(cs), 0.03, P(state), P(kl), _st()), "kl")
        _ok(L.navppo_adam_step_clipped(P(pc), P(gc), P(mc), P(vc), n, n_first, 0.5, max_norm, *HYPER, step, P(csc), _st()), "clipped")
        torch.cuda.synchronize()
        assert state.tolist() == [0.0, 1.0, 0.0, 0.0]
        _check_adam(p0, m0, v0, g, step, p, m, v, what=f"adam_step_kl n={n} n_first={n_first} step={step}")
        for x, y in ((p, pc), (g, gc), (m, mc), (v, vc), (cs, csc)):
            assert torch.equal(x, y)
        # above the limit (and a NaN): nothing moves
        for bad_kl in (0.031, float("nan")):
            p, g, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
            cs, state = torch.full((4,), -7.0, device=DEV), torch.zeros(4, device=DEV)
            klb = torch.tensor([bad_kl], device=DEV)
            _ok(L.navppo_adam_step_kl(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step, P(cs), 0.03, P(state), P(klb), _st()), "kl")
            torch.cuda.synchronize()
            for x, x0 in ((p, p0), (g, g0), (m, m0), (v, v0)):
                assert torch.equal(x.cpu(), x0)
            assert torch.equal(cs[:2], csc[:2]) and cs[2:].tolist() == [0.0, 0.0]
            st = state.tolist()
            assert st[0] == 1.0 and st[1] == 0.0 and st[3] == float(step)
            assert math.isnan(st[2]) if math.isnan(bad_kl) else st[2] == float(klb[0])
            cs.fill_(-7.0)   # stopped: the norm launch and the step launch return at their entry
            _ok(L.navppo_adam_step_kl(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step + 1, P(cs), 0.03, P(state), P(kl), _st()), "kl")
            torch.cuda.synchronize()
            assert torch.equal(p.cpu(), p0) and bool((cs == -7.0).all()) and state.tolist()[3] == float(step)


def _trainer(policy, n_ep, target_kl=None, iters=1):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(256, map="stage_1", max_episode_steps=40, seed=1)
    cfg = ppo.PPOConfig(rollout_len=64, max_episode_steps=40, n_updates_per_iteration=n_ep, policy=policy, seed=2, target_kl=target_kl)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.updater.fused
    logs = [dict(tr.iteration()) for _ in range(iters)]
    torch.cuda.synchronize()
    out = dict(flat=tr.updater.fp.flat.clone(), m=tr.updater._adam_m.clone(), v=tr.updater._adam_v.clone(), t=tr.updater._adam_t,
               kls=tr.updater._fhist[:n_ep, 1].tolist(), hist=tr.updater.loss_history.clone(), logs=logs, tb=tr.tb_scalars())
    env.close()
    return out


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_stops_where_the_devices_kl_says(policy):
    """Run A (no target) yields the per-epoch approx_kl; run B (same seeds, the target in the gap) stops there and leaves exactly the
    weights and moments of run C, which was only asked for that many epochs."""
    A = _trainer(policy, 6)
    kls = A["kls"]
    j = next((k for k in range(3, 7) if kls[k - 1] > 1.5 * max(kls[:k - 1])), None)
    print(f"{policy}: approx_kl of epochs 1..6 = {kls}, j = {j}")
    assert j is not None, kls
    target = 0.5 * (max(kls[:j - 1]) + kls[j - 1]) / 1.5
    B = _trainer(policy, 6, target_kl=target, iters=2)
    lg = B["logs"][0]
    assert lg["kl_stop_epoch"] == j - 1 and lg["kl_stopped"] == 1
    assert "skipped_steps_actor" not in lg                     # (no max_grad_norm: the keys of the unclipped statistics)
    assert lg["approx_kl"] == pytest.approx(sum(kls[:j]) / j, rel=1e-5, abs=1e-12)   # means over the j epochs whose passes ran
    lg2 = B["logs"][1]                                         # a second iteration runs and stays finite
    assert 0 <= lg2["kl_stop_epoch"] <= 6 and bool(torch.isfinite(B["flat"]).all()) and math.isfinite(lg2["actor_loss"])
    assert B["t"] == (j - 1) + lg2["kl_stop_epoch"]
    assert B["tb"]["ppo/kl_stop_epoch"] == lg2["kl_stop_epoch"] and B["tb"]["ppo/kl_stopped"] == lg2["kl_stopped"]
    B1 = _trainer(policy, 6, target_kl=target)
    C_ = _trainer(policy, j - 1)
    for k in ("flat", "m", "v"):
        assert torch.equal(B1[k], C_[k]), k
    assert B1["t"] == j - 1 == C_["t"]
    assert bool(torch.isfinite(B1["hist"][:j]).all()) and bool(torch.isnan(B1["hist"][j:]).all())
    assert torch.equal(B1["hist"][:j - 1], C_["hist"])


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_with_clipping_does_not_count_the_trip_as_a_skipped_step(policy):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(256, map="stage_1", max_episode_steps=40, seed=1)
    cfg = ppo.PPOConfig(rollout_len=64, max_episode_steps=40, n_updates_per_iteration=6, policy=policy, seed=2, target_kl=1e-9,
                        max_grad_norm=0.5)
    tr = ppo.PPOTrainer(env, cfg)
    lg = tr.iteration()   # epoch 1 has approx_kl ~ 0 (the rollout's own policy); the first moved policy is over 1.5e-9
    assert lg["kl_stopped"] == 1 and 0 <= lg["kl_stop_epoch"] <= 2, lg
    assert lg["skipped_steps_actor"] == 0 and lg["skipped_steps_critic"] == 0
    k = lg["kl_stop_epoch"] + 1
    cs = tr.updater.clip_stats.cpu()
    assert cs[k - 1, 2:].tolist() == [0.0, 0.0] and bool(torch.isfinite(cs[:k, :2]).all()) and bool((cs[:k, :2] > 0).all())
    assert lg["grad_clip_frac_critic"] == pytest.approx(float((cs[:k - 1, 3] < 1).float().sum()) / k)
    env.close()


def _dp_kl_worker(rank, world, port, path, policy, target_kl):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduces here
    from navbot_ppo_amd import ppo
    from navbot_ppo_amd.env import VecEnv
    ctx = ppo.DistCtx(device="cuda:0")
    lo, hi = ctx.shard(128)
    env = VecEnv(hi - lo, map="stage_1", max_episode_steps=20, seed=3, env_id_base=lo, device="cuda:0")
    cfg = ppo.PPOConfig(rollout_len=32, max_episode_steps=20, n_updates_per_iteration=5, policy=policy, seed=5, target_kl=target_kl)
    tr = ppo.PPOTrainer(env, cfg, ctx)
    lg = tr.iteration()
    torch.cuda.synchronize()
    torch.save({"flat": tr.updater.fp.flat.cpu(), "m": tr.updater._adam_m.cpu(), "state": tr.updater.kl_state.cpu(), "t": tr.updater._adam_t,
                "keys": {k: lg[k] for k in ("kl_stop_epoch", "kl_stopped", "approx_kl")}}, f"{path}.{rank}")
    ctx.barrier()
    env.close()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_two_ranks_stop_at_the_same_epoch(tmp_path, policy):
    """Two gloo ranks sharing the GPU: ungated passes -> all-reduce of the gradient and of [kl n, n] -> navppo_adam_step_kl.  The ranks'
    shards differ, the global approx_kl does not: both stop at the same epoch with equal weights."""
    from _ranks import spawn_ranks
    path = str(tmp_path / "dpkl")
    spawn_ranks(_dp_kl_worker, 2, lambda port: (2, port, path, policy, 1e-9))
    r0, r1 = torch.load(path + ".0"), torch.load(path + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["m"], r1["m"]) and bool(torch.isfinite(r0["flat"]).all())
    assert torch.equal(r0["state"], r1["state"]) and r0["keys"] == r1["keys"]
    assert r0["keys"]["kl_stopped"] == 1 and 0 <= r0["keys"]["kl_stop_epoch"] <= 2
    assert r0["t"] == r1["t"] == r0["keys"]["kl_stop_epoch"] == int(r0["state"][1])
