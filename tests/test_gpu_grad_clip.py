"""Gradient-norm clipping and the non-finite guard inside the fused PPO update (navppo_*_update_epoch_clipped,
navppo_adam_step_clipped, PPOConfig.max_grad_norm) on the GPU, for every family of fused kernels: the 2x64 heads on the f32-input
MFMA at 16 and 42 columns, on split-bf16 products at 16 and 42 columns, on float16 rows (a ragged batch), and the 512-wide nets.

Adam is almost invariant to a constant gradient scale, so the parameters alone do not show a clip: the tests look at the
coefficients, the clipped gradient and Adam's moments."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd._native import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
INF = float("inf")
U = 2.0 ** -24     # float32 unit roundoff; one ulp of x is at most 2 U |x|
HYPER = (3e-4, 0.9, 0.999, 1e-8)
F32 = lambda x: float(np.float32(x))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    assert rc == 0, f"{what}: rc {rc}: {lib().navppo_last_error().decode()}"


class Family:
    """One family of fused kernels on one batch: start weights, the unclipped gradient (*_loss_grad) and epochs, unclipped or clipped,
    on explicit (params, m, v) state."""

    def __init__(self, kind, D, f16, n, seed=11):
        self.kind, self.D, self.f16, self.n = kind, D, f16, n
        self.L = lib()
        torch.manual_seed(seed)
        a, c = nets.make_policy("resmlp512" if kind == "resmlp" else "mlp64x2", **({} if kind == "resmlp" else dict(obs_dim=D)))
        fp = [p for m in (a, c) for k, p in m.named_parameters() if ".bn" not in "." + k and not k.startswith("bn")]
        self.flat = torch.cat([p.detach().reshape(-1) for p in fp]).contiguous().to(DEV)
        self.PA = 50290 if kind == "resmlp" else 64 * D + 4354
        self.PT = self.flat.numel()
        g = torch.Generator().manual_seed(seed + 1)
        obs = torch.rand((n, D), generator=g)
        acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
        logp = -1.2 - 2.3 * torch.rand(n, generator=g)
        rtg = torch.randn(n, generator=g) * 3
        adv = torch.randn(n, generator=g)
        self.obs, self.acts, self.logp, self.rtg, self.adv = [t.to(DEV).contiguous() for t in (obs, acts, logp, rtg, adv)]
        if f16:
            self.obs = self.obs.half()
        ws_bytes = self.L.navppo_resmlp512_workspace_bytes(n) + 16 if kind == "resmlp" else self.L.navppo_mlp64_workspace_bytes(D)
        self.ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=DEV)
        self.prep = None
        self.m0 = (torch.rand(self.PT, generator=g) * 1e-3 - 5e-4).to(DEV)     # a used optimiser: "unchanged" means something
        self.v0 = (torch.rand(self.PT, generator=g) * 1e-6).to(DEV)

    def _oargs(self, obs):
        if self.kind == "x3":
            nb = self.L.navppo_mlp64_bf16x3_prep_bytes(self.n, self.D)
            self.prep = torch.empty(nb, dtype=torch.uint8, device=DEV)
            _ok(self.L.navppo_mlp64_bf16x3_prepare(P(obs), self.D, self.f16, self.n, P(self.prep), _st()), "prepare")
            return (P(self.prep), self.D)
        return (P(obs), self.f16) if self.kind == "resmlp" else (P(obs), self.D, self.f16)

    @property
    def prefix(self):
        return {"mlp64": "navppo_mlp64_", "x3": "navppo_mlp64_bf16x3_", "resmlp": "navppo_resmlp512_"}[self.kind]

    def loss_grad(self, params, rtg=None, obs=None):
        gr = torch.zeros(self.PT, device=DEV)
        st = torch.zeros(8, device=DEV)
        _ok(getattr(self.L, self.prefix + "loss_grad")(P(params), *self._oargs(self.obs if obs is None else obs), P(self.acts), P(self.logp),
                                                       P(self.rtg if rtg is None else rtg), P(self.adv), self.n, 0.6, 0.2, P(gr), P(st),
                                                       P(self.ws), _st()), self.prefix + "loss_grad")
        torch.cuda.synchronize()
        return gr

    def start(self, used=False):
        return dict(p=self.flat.clone(), m=self.m0.clone() if used else torch.zeros_like(self.flat),
                    v=self.v0.clone() if used else torch.zeros_like(self.flat), g=torch.zeros_like(self.flat), st=torch.zeros(8, device=DEV))

    def epoch(self, s, step, max_norm=None, rtg=None, obs=None):
        """One epoch in place on state s; max_norm None: the existing *_update_epoch.  Returns clip_stats [4] (clipped) or None."""
        cs = None if max_norm is None else torch.full((4,), -7.0, device=DEV)
        tail = () if max_norm is None else (max_norm, P(cs))
        name = self.prefix + ("update_epoch" if max_norm is None else "update_epoch_clipped")
        _ok(getattr(self.L, name)(P(s["p"]), *self._oargs(self.obs if obs is None else obs), P(self.acts), P(self.logp),
                                  P(self.rtg if rtg is None else rtg), P(self.adv), self.n, 0.6, 0.2, *HYPER, step, P(s["m"]), P(s["v"]),
                                  P(s["g"]), P(s["st"]), P(self.ws), *tail, _st()), name)
        torch.cuda.synchronize()
        return cs

    def nets_of(self, t):
        return t[:self.PA], t[self.PA:]


# every family; float16 rows on a ragged batch
FAMILIES = [("mlp64", 16, 0, 4096), ("mlp64", 42, 0, 4096), ("mlp64", 16, 1, 3001), ("x3", 16, 0, 4096), ("x3", 42, 0, 4096),
            ("x3", 16, 0, 2 * 4096 + 37), ("resmlp", 16, 0, 4096)]
fam_ids = [f"{k}-d{d}-{'f16' if h else 'f32'}-n{n}" for k, d, h, n in FAMILIES]


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("p", "m", "v", "g"))


def _check_adam(p0, m0, v0, g, step, p1, m1, v1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, what=""):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64 from the float32 state and gradient g; the kernel's (p1, m1, v1)
    within a few float32 ulps of the terms of each update -- the bounds of tests/test_gpu_tails.py's check of the unclipped epoch."""
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    p0, m0, v0, g = (t.double().cpu() for t in (p0, m0, v0, g))
    p1, m1, v1 = (t.double().cpu() for t in (p1, m1, v1))
    mr = m0 + (g - m0) * (1 - b1)
    vr = b2 * v0 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (lr / bc1) * mr / (vr.sqrt() / math.sqrt(bc2) + eps)
    pr = p0 - upd
    tiny = 2.0 ** -124
    dm = 4 * U * (b1 * m0.abs() + (1 - b1) * g.abs()) + tiny
    assert bool(((m1 - mr).abs() <= dm).all()), (what, "m", (m1 - mr).abs().max().item())
    assert bool(((v1 - vr).abs() <= 4 * U * vr + tiny).all()), (what, "v")
    err = (p1 - pr).abs()
    bound = 2 * U * pr.abs() + 12 * U * upd.abs() + (lr / bc1) * dm / (vr.sqrt() / math.sqrt(bc2) + eps) + tiny
    bad = err > bound
    assert not bool(bad.any()), (what, "params", int(bad.sum()), (err / bound.clamp_min(1e-300)).max().item(), step)


def _check_clip(fam, g_unclipped, cs, max_norm, what):
    """clip_stats of one call against float64 on that epoch's unclipped gradient: the squared norms within 2e-4 relative (the bound
    of 64 + 1600 sequential float32 additions, the longest chain either reduction has), the coefficients within 1e-4 relative of
    min(1, max_norm / (norm + 1e-6)).  Returns the kernel's coefficients."""
    cs = cs.double().cpu()
    out = []
    for k, g in enumerate(fam.nets_of(g_unclipped.double().cpu())):
        s64 = float((g * g).sum())
        print(f"{what} net {k}: s {float(cs[k]):.9g} (float64 {s64:.9g}), coef {float(cs[2 + k]):.9g}")
        assert abs(float(cs[k]) - s64) <= 2e-4 * s64, (what, k, float(cs[k]), s64)
        want = min(1.0, max_norm / (math.sqrt(s64) + 1e-6))
        assert abs(float(cs[2 + k]) - want) <= 1e-4 * want, (what, k, float(cs[2 + k]), want)
        out.append(float(cs[2 + k]))
    return out


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_infinite_bound_is_the_existing_epoch(kind, D, f16, n):
    """Five clipped epochs with max_norm = +inf == five epochs of *_update_epoch from the same start, bit for bit (params, both moments,
    the gradient output); every coefficient exactly 1."""
    fam = Family(kind, D, f16, n)
    a, b = fam.start(), fam.start()
    for step in range(1, 6):
        cs = fam.epoch(a, step, INF)
        fam.epoch(b, step)
        assert _same(a, b), (fam_ids, step)
        assert torch.equal(cs[2:].cpu(), torch.ones(2)), cs
        assert torch.equal(a["st"][[0, 1, 2, 4]], b["st"][[0, 1, 2, 4]])
        g64 = a["g"].double()
        for k, g in enumerate(fam.nets_of(g64)):
            s64 = float((g * g).sum())
            assert abs(float(cs[k]) - s64) <= 2e-4 * s64
    assert not torch.equal(a["p"], fam.flat)


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_clip_engages_and_is_torchs(kind, D, f16, n):
    """max_norm = half the SMALLER net's measured norm: both nets clip.  Three epochs; after each, the statistics against float64 on the
    unclipped gradient of that epoch's weights, the gradient output = coef x g within 2 ulp, and params / m / v against float64 Adam
    fed that output.  After the first epoch m_clipped / m_unclipped = coef: what a missing clip breaks (the parameters would not show it)."""
    fam = Family(kind, D, f16, n)
    g0 = fam.loss_grad(fam.flat)
    norms = [float(g.double().norm()) for g in fam.nets_of(g0)]
    assert all(x > 0 and math.isfinite(x) for x in norms), norms
    max_norm = F32(0.5 * min(norms))
    s = fam.start()
    ref = fam.start()
    fam.epoch(ref, 1)                                  # the unclipped first epoch
    for step in (1, 2, 3):
        g = fam.loss_grad(s["p"])                      # this epoch's unclipped gradient (same kernels, same order: the same bits)
        before = {k: s[k].clone() for k in ("p", "m", "v")}
        cs = fam.epoch(s, step, max_norm)
        coefs = _check_clip(fam, g, cs, max_norm, f"{kind} d{D} step {step}")
        if step == 1:
            assert coefs[0] < 1.0 and coefs[1] < 1.0, coefs
        for k, (gk, gd) in enumerate(zip(fam.nets_of(g), fam.nets_of(s["g"]))):
            want = gk.double() * float(cs[2 + k])      # the kernel's own float32 coefficient
            assert bool(((gd.double() - want).abs() <= 2 * (2 * U) * want.abs() + 2.0 ** -140).all()), (kind, step, k)
        _check_adam(before["p"], before["m"], before["v"], s["g"], step, s["p"], s["m"], s["v"], what=f"{kind} d{D} step {step}")
        if step == 1:
            for k, (mc, mu) in enumerate(zip(fam.nets_of(s["m"]), fam.nets_of(ref["m"]))):
                big = mu.abs() > 1e-3 * mu.abs().max()
                ratio = (mc[big].double() / mu[big].double()).cpu().numpy()
                # m = fl(fl(g c) fl(1 - beta1)) against fl(g fl(1 - beta1)): three roundings apart
                np.testing.assert_allclose(ratio, coefs[k], rtol=8 * U)
                assert int(big.sum()) > 100


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_bound_above_the_norm_does_not_clip(kind, D, f16, n):
    fam = Family(kind, D, f16, n)
    g0 = fam.loss_grad(fam.flat)
    max_norm = F32(2.0 * max(float(g.double().norm()) for g in fam.nets_of(g0)))
    a, b = fam.start(used=True), fam.start(used=True)
    cs = fam.epoch(a, 4, max_norm)
    fam.epoch(b, 4)
    assert torch.equal(cs[2:].cpu(), torch.ones(2)), cs
    assert _same(a, b)


@pytest.mark.parametrize("kind,D,f16,n", FAMILIES, ids=fam_ids)
def test_non_finite_gradient_skips_that_net_only(kind, D, f16, n):
    """One NaN in rtg: the critic's gradient is not finite, the actor's is bit-identical to the clean run's -> coef_critic == 0, the
    critic's params / m / v bit-unchanged, the actor's slices those of the clean clipped epoch.  One NaN observation: both nets skip."""
    fam = Family(kind, D, f16, n)
    g0 = fam.loss_grad(fam.flat)
    max_norm = F32(0.5 * min(float(g.double().norm()) for g in fam.nets_of(g0)))
    rtg_bad = fam.rtg.clone()
    rtg_bad[n // 3] = float("nan")
    gb = fam.loss_grad(fam.flat, rtg=rtg_bad)
    assert torch.equal(gb[:fam.PA], g0[:fam.PA]) and not bool(torch.isfinite(gb[fam.PA:]).all())
    clean, bad = fam.start(used=True), fam.start(used=True)
    cs_clean = fam.epoch(clean, 3, max_norm)
    cs = fam.epoch(bad, 3, max_norm, rtg=rtg_bad)
    PA = fam.PA
    assert float(cs[3]) == 0.0 and not math.isfinite(float(cs[1])), cs
    assert float(cs[2]) == float(cs_clean[2]) and float(cs[0]) == float(cs_clean[0])
    for k, t0 in (("p", fam.flat), ("m", fam.m0), ("v", fam.v0)):
        assert torch.equal(bad[k][PA:], t0[PA:]), k
        assert torch.equal(bad[k][:PA], clean[k][:PA]) and not torch.equal(bad[k][:PA], t0[:PA]), k
    assert torch.equal(bad["g"][:PA], clean["g"][:PA])
    obs_bad = fam.obs.clone()
    obs_bad[n // 2, 3] = float("nan")
    both = fam.start(used=True)
    cs = fam.epoch(both, 3, max_norm, obs=obs_bad)
    assert float(cs[2]) == 0.0 and float(cs[3]) == 0.0, cs
    for k, t0 in (("p", fam.flat), ("m", fam.m0), ("v", fam.v0)):
        assert torch.equal(both[k], t0), k


@pytest.mark.parametrize("kind,D,f16", [("mlp64", 16, 0), ("x3", 42, 0), ("resmlp", 16, 0)])
def test_clipped_entry_points_check_their_arguments(kind, D, f16):
    fam = Family(kind, D, f16, 256)
    s = fam.start()
    L = lib()
    name = fam.prefix + "update_epoch_clipped"

    def call(max_norm, cs):
        return getattr(L, name)(P(s["p"]), *fam._oargs(fam.obs), P(fam.acts), P(fam.logp), P(fam.rtg), P(fam.adv), fam.n, 0.6, 0.2, *HYPER, 1,
                                P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(fam.ws), max_norm, P(cs), _st())
    cs = torch.zeros(4, device=DEV)
    for bad in (0.0, -1.0, float("nan")):
        assert call(bad, cs) == -1 and b"max_norm" in L.navppo_last_error()
    assert call(1.0, None) == -1 and L.navppo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(s["p"], fam.flat) and call(1.0, cs) == 0
    t = torch.zeros(64, device=DEV)
    for bad in (0.0, -1.0, float("nan")):
        assert L.navppo_adam_step_clipped(P(t), P(t), P(t), P(t), 64, 32, 0.5, bad, *HYPER, 1, P(cs), _st()) == -1
    assert L.navppo_adam_step_clipped(P(t), P(t), P(t), P(t), 64, 32, 0.5, 1.0, *HYPER, 1, None, _st()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,n_first", [(5378 + 5313, 5378), (50290 + 50257, 50290), (5378, 5378), (5313, 0), (257, 100)])
def test_adam_step_clipped_against_float64(n, n_first):
    """The multi-GPU form on an all-reduced sum with grad_scale = 1/2: norms of the SCALED gradient per segment, coefficient, clipped
    gradient output and Adam against float64 -- at the segment boundaries of both policies, with one segment empty (the per-net steps
    of the pipelined epoch) and off the block size; then a NaN in the second segment skips that segment only."""
    L = lib()
    gen = torch.Generator().manual_seed(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.05
    g0[n_first:] *= 7.0
    m0, v0 = torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-6
    gs = g0.double() * 0.5
    segs = [slice(0, n_first), slice(n_first, n)]
    norms = [float(gs[sl].norm()) for sl in segs]
    for max_norm, step in ((F32(0.5 * min(x for x in norms if x > 0)), 1), (F32(2 * max(norms)), 7), (INF, 2)):
        p, g, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
        cs = torch.full((4,), -7.0, device=DEV)
        _ok(L.navppo_adam_step_clipped(P(p), P(g), P(m), P(v), n, n_first, 0.5, max_norm, *HYPER, step, P(cs), _st()), "adam_step_clipped")
        torch.cuda.synchronize()
        c = cs.double().cpu()
        for k, sl in enumerate(segs):
            s64 = float((gs[sl] * gs[sl]).sum())
            want = min(1.0, max_norm / (math.sqrt(s64) + 1e-6))
            assert abs(float(c[k]) - s64) <= 2e-4 * s64 and abs(float(c[2 + k]) - want) <= 1e-4 * want, (k, c, s64, want)
            if sl.stop > sl.start:
                assert (float(c[2 + k]) < 1.0) == (max_norm < norms[k])
            exp = gs[sl] * float(c[2 + k])
            assert bool(((g.double().cpu()[sl] - exp).abs() <= 2 * (2 * U) * exp.abs() + 2.0 ** -140).all())
        _check_adam(p0, m0, v0, g, step, p, m, v, what=f"adam_step_clipped n={n} n_first={n_first} step={step}")
    if 0 < n_first < n:
        gb = g0.clone()
        gb[n - 1] = float("nan")
        p, g, m, v = (t.clone().to(DEV) for t in (p0, gb, m0, v0))
        cs = torch.full((4,), -7.0, device=DEV)
        _ok(L.navppo_adam_step_clipped(P(p), P(g), P(m), P(v), n, n_first, 0.5, 1.0, *HYPER, 3, P(cs), _st()), "adam_step_clipped")
        torch.cuda.synchronize()
        assert float(cs[3]) == 0.0 and float(cs[2]) > 0.0
        for t, t0 in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(t.cpu()[n_first:], t0[n_first:]) and not torch.equal(t.cpu()[:n_first], t0[:n_first])


def _dp_clip_worker(rank, world, port, path, policy, overlap):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduce here
    from navbot_ppo_amd import ppo
    from navbot_ppo_amd.env import VecEnv
    ctx = ppo.DistCtx(device="cuda:0")
    lo, hi = ctx.shard(128)
    env = VecEnv(hi - lo, map="stage_1", max_episode_steps=20, seed=3, env_id_base=lo, device="cuda:0")
    cfg = ppo.PPOConfig(rollout_len=32, max_episode_steps=20, n_updates_per_iteration=3, policy=policy, seed=5, max_grad_norm=0.05,
                        overlap_allreduce=overlap)
    tr = ppo.PPOTrainer(env, cfg, ctx)
    lg = tr.iteration()
    torch.cuda.synchronize()
    torch.save({"flat": tr.updater.fp.flat.cpu(), "clip": tr.updater.clip_stats.cpu(), "m": tr.updater._adam_m.cpu(),
                "keys": {k: lg[k] for k in ("grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic",
                                            "actor_grad_norm", "critic_grad_norm")}}, f"{path}.{rank}")
    ctx.barrier()
    env.close()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("policy,overlap", [("mlp64x2", False), ("mlp64x2", True), ("resmlp512", False)])
def test_two_rank_trainer_clips_identically_on_both_ranks(tmp_path, policy, overlap):
    """PPOTrainer(PPOConfig(max_grad_norm=...)) on two gloo ranks sharing the GPU: fused passes -> all-reduce -> navppo_adam_step_clipped
    (plain and per-net pipeline).  Weights and clip statistics equal on both ranks; the critic (norm far above the bound) clips."""
    from _ranks import spawn_ranks
    path = str(tmp_path / "dpclip")
    spawn_ranks(_dp_clip_worker, 2, lambda port: (2, port, path, policy, overlap))
    r0, r1 = torch.load(path + ".0"), torch.load(path + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["m"], r1["m"]) and bool(torch.isfinite(r0["flat"]).all())
    assert torch.equal(r0["clip"], r1["clip"]) and r0["clip"].shape == (3, 4)
    assert bool((r0["clip"][:, 3] < 1.0).all()) and bool((r0["clip"][:, 2:] > 0.0).all()) and bool((r0["clip"][:, :2] > 0).all())
    assert r0["keys"] == r1["keys"] and r0["keys"]["grad_clip_frac_critic"] == 1.0 and r0["keys"]["skipped_steps_actor"] == 0
    np.testing.assert_allclose(r0["keys"]["critic_grad_norm"], float(r0["clip"][:, 1].sqrt().mean()), rtol=1e-5)


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_end_to_end_with_clipping_and_a_planted_nan(policy, tmp_path, capsys):
    """Two iterations with max_grad_norm set: the new keys, clip fractions in [0, 1], finite weights.  Then a NaN planted in the rollout
    buffers before the update: the warning, grad_diagnostics.txt with its fields, every step of both nets skipped, weights unchanged."""
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(256, map="stage_1", max_episode_steps=40, seed=1)
    cfg = ppo.PPOConfig(rollout_len=64, max_episode_steps=40, n_updates_per_iteration=4, policy=policy, seed=2, max_grad_norm=0.5,
                        output_dir=str(tmp_path), episode_csv_rows=0, tb_episode_rows=0, save_freq=1000)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.updater.fused
    for _ in range(2):
        lg = tr.iteration()
        for k in ("grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic"):
            assert k in lg and k in tr.updater.stats
        assert 0.0 <= lg["grad_clip_frac_actor"] <= 1.0 and 0.0 <= lg["grad_clip_frac_critic"] <= 1.0
        assert lg["skipped_steps_actor"] == 0 and lg["skipped_steps_critic"] == 0
        assert lg["actor_grad_norm"] > 0 and lg["critic_grad_norm"] > 0
        cs = tr.updater.clip_stats.cpu()
        assert cs.shape == (4, 4) and lg["critic_grad_norm"] == pytest.approx(float(cs[:, 1].sqrt().mean()), rel=1e-5)
        assert lg["grad_clip_frac_critic"] == pytest.approx(float((cs[:, 3] < 1).float().mean()))
    assert bool(torch.isfinite(tr.updater.fp.flat).all())
    sc = tr.tb_scalars()
    assert {"ppo/grad_clip_frac_actor", "ppo/grad_clip_frac_critic", "ppo/skipped_steps_actor", "ppo/skipped_steps_critic"} <= set(sc)
    assert not os.path.exists(os.path.join(str(tmp_path), "grad_diagnostics.txt"))
    capsys.readouterr()
    rollout = tr.rollout

    def rollout_then_nan():
        rollout()
        tr.obs_buf[3, 5, 2] = float("nan")
    tr.rollout = rollout_then_nan
    before = tr.updater.fp.flat.clone()
    m_before = tr.updater._adam_m.clone()
    lg = tr.iteration()
    out = capsys.readouterr().out
    assert "[WARNING] Actor grad norm invalid:" in out and "[WARNING] Critic grad norm invalid:" in out
    assert f"at iteration {lg['iteration']}. Check grad_diagnostics.txt" in out
    txt = open(os.path.join(str(tmp_path), "grad_diagnostics.txt")).read()
    for field in (f"Iteration {lg['iteration']}", "Net: actor", "Net: critic", "grad norm:", "loss:", "Skipped steps: 4 of 4",
                  "Advantage stats: mean=", "std=", "min=", "max=", "Clip fraction:"):
        assert field in txt, field
    assert lg["skipped_steps_actor"] == 4 and lg["skipped_steps_critic"] == 4
    assert torch.equal(tr.updater.fp.flat, before) and torch.equal(tr.updater._adam_m, m_before)
    env.close()
