"""The learned exploration variance on the GPU (navppo_*_update_epoch_var, PPOConfig.learn_var), for every family of fused kernels at
the shapes of tests/test_gpu_grad_clip.py and at the batch tails of tests/test_gpu_tails.py:

  1. the nets' step of a *_var call is bit for bit the clipped (or adaptive-rate) epoch's called with the state's variance by value;
  2. d/d(log var) against float64 autograd of the surrogate minus ent_coef * entropy, held to 2.5 x the error of PyTorch's float32;
  3. eight queued calls against a replay on the host through ppo.learned_var_reference;
  4. the exact corners (zero advantages, both clamps, a NaN advantage, repeatability);
  5. every refusal of the entry points;
  6. the trainer: the logged variance is the mirror's, the next rollout draws with it, a checkpoint restores it."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import test_gpu_grad_clip as gc
from _guards import run_both
from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd.explore_var import ADAM_M, ADAM_V, ENTROPY, GRAD, SKIPPED, STEPS, THETA, VAR

pytestmark = pytest.mark.gpu
DEV = gc.DEV
INF = float("inf")
P, _st, _ok, HYPER, F32 = gc.P, gc._st, gc._ok, gc.HYPER, gc.F32
LOG_2PI = math.log(2.0 * math.pi)
FULL_MANTISSA = F32(0.37283847)   # a variance whose float32 has bits down to the last place
PREFIX = {"mlp64": "navppo_mlp64_", "x3": "navppo_mlp64_bf16x3_", "resmlp": "navppo_resmlp512_"}
LR_ARGS = (0.01, 1e-5, 1e-2)   # kl_target, lr_min, lr_max


def vstate(var):
    return torch.tensor(ppo.var_state_init(var), dtype=torch.float32, device=DEV)


class VFamily(gc.Family):
    """gc.Family with its nets kept (for the float64 / float32 autograd references) and epochs that take the variance explicitly."""

    def __init__(self, kind, D, f16, n, seed=11):
        torch.manual_seed(seed)   # (the parent seeds and builds the same way: the same weights)
        self.actor, self.critic = nets.make_policy("resmlp512" if kind == "resmlp" else "mlp64x2", **({} if kind == "resmlp" else dict(obs_dim=D)))
        super().__init__(kind, D, f16, n, seed)
        fp = [p for m in (self.actor, self.critic) for k, p in m.named_parameters() if ".bn" not in "." + k and not k.startswith("bn")]
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in fp]).to(DEV), self.flat)
        self._oa = None

    def oargs(self):
        if self._oa is None:   # (x3: the rows are split once)
            self._oa = self._oargs(self.obs)
        return self._oa

    def epoch(self, s, step, var, max_norm, cs, lr_state=None, adapt=0, lr=HYPER[0], adv=None):
        """*_update_epoch_clipped (lr_state None) or *_update_epoch_lr with `var` by value, in place on s; no synchronisation"""
        tail = (max_norm, P(cs)) + (() if lr_state is None else (*LR_ARGS, adapt, P(lr_state)))
        name = self.prefix + ("update_epoch_clipped" if lr_state is None else "update_epoch_lr")
        _ok(getattr(self.L, name)(P(s["p"]), *self.oargs(), P(self.acts), P(self.logp), P(self.rtg), P(self.adv if adv is None else adv), self.n,
                                  var, 0.2, lr, *HYPER[1:], step, P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(self.ws), *tail, _st()), name)

    def epoch_var(self, s, step, vs, max_norm, cs, lr_state=None, adapt=0, lr=HYPER[0], ent_coef=0.0, var_min=1e-3, var_max=1.0, adv=None,
                  logp=None):
        """*_update_epoch_var on the variance state vs, in place on s; no synchronisation"""
        name = self.prefix + "update_epoch_var"
        _ok(getattr(self.L, name)(P(s["p"]), *self.oargs(), P(self.acts), P(self.logp if logp is None else logp), P(self.rtg),
                                  P(self.adv if adv is None else adv), self.n, 0.2, lr, *HYPER[1:], step, P(s["m"]), P(s["v"]), P(s["g"]),
                                  P(s["st"]), P(self.ws), max_norm, P(cs), *LR_ARGS, adapt, P(lr_state), ent_coef, var_min, var_max, P(vs),
                                  _st()), name)


def _cs():
    return torch.full((4,), -7.0, device=DEV)


# ================================================================================================ 1: the nets' step is the clipped epoch's
@pytest.mark.parametrize("kind,D,f16,n", gc.FAMILIES, ids=gc.fam_ids)
@pytest.mark.parametrize("var", [0.6, FULL_MANTISSA], ids=["var0.6", "var_full_mantissa"])
def test_the_nets_step_is_the_clipped_epochs_bit_for_bit(kind, D, f16, n, var):
    fam = VFamily(kind, D, f16, n)
    for adaptive in (False, True):
        a, b = fam.start(used=True), fam.start(used=True)
        vs = vstate(var)
        lra = torch.tensor([1e-3, 1e-3, 0, 0], device=DEV) if adaptive else None
        lrb = None if lra is None else lra.clone()
        for step in (1, 2):   # (the second step: the variance the first one left)
            v_now = float(vs[VAR])
            assert step > 1 or v_now == F32(var)
            ca, cb = _cs(), _cs()
            fam.epoch(a, step, v_now, 0.5, ca, lra, adapt=int(step > 1))
            fam.epoch_var(b, step, vs, 0.5, cb, lrb, adapt=int(step > 1), ent_coef=0.01)
            torch.cuda.synchronize()
            what = f"{kind} adaptive={adaptive} step={step}"
            assert gc._same(a, b), what
            assert torch.equal(ca, cb), what
            assert torch.equal(a["st"][[0, 1, 2, 4]], b["st"][[0, 1, 2, 4]]), what
            if adaptive:
                assert torch.equal(lra, lrb), what
        st = vs.tolist()
        assert st[STEPS] == 2.0 and st[SKIPPED] == 0.0 and st[VAR] != F32(var)


# ================================================================================================ 2: d/d(log var) against float64
def _theta_grad(actor, obs, acts, logp, adv, var, ent_coef, dtype):
    """autograd of the reference's surrogate (ppo.py:316-342) minus ent_coef x entropy with respect to theta = log var, on the CPU.
    Returns (the gradient, the ratios, the mask of samples whose clipped branch is the minimum: no gradient flows through them)."""
    a = copy.deepcopy(actor).cpu().to(dtype)
    obs, acts, logp, adv = (t.detach().cpu().to(dtype) for t in (obs.float() if dtype == torch.float32 else obs, acts, logp, adv))
    theta = torch.tensor(math.log(var), dtype=dtype, requires_grad=True)
    lp = ppo.gaussian_log_prob(a(obs), acts, torch.exp(theta))
    ratio = torch.exp(lp - logp)
    s1, s2 = ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv
    loss = (-torch.min(s1, s2)).mean() - ent_coef * (1.0 + LOG_2PI + theta)
    loss.backward()
    inside = (ratio >= 0.8) & (ratio <= 1.2)
    return float(theta.grad), ratio.detach(), ~(inside | (s1 < s2)).detach()


def _kink_free_batch(fam, var, seed):
    """logp_old = the policy's own log-probability (float64) plus a perturbation, so that the ratios spread over both sides of the clip
    range; then the samples near a kink are replaced in place (the 2x64 heads: tests/_kinks.py, relu units and clip boundaries; the
    512-wide nets, which that helper does not know: the clip boundaries, by the same rule -- the value of d/d(log var) is continuous
    across a unit's kink, not across a clip boundary), so that float32 and float64 take the same branch."""
    from _kinks import replace_kink_samples
    g = torch.Generator().manual_seed(1000 + seed)
    a64 = copy.deepcopy(fam.actor).cpu().double()
    v = torch.tensor(F32(var), dtype=torch.float64)
    with torch.no_grad():
        lp = ppo.gaussian_log_prob(a64(fam.obs.cpu().double()), fam.acts.cpu().double(), v)
        logp = (lp + (torch.rand(fam.n, generator=g, dtype=torch.float64) - 0.5) * 0.8).float().to(DEV).contiguous()
        if fam.kind != "resmlp":
            replace_kink_samples(fam.actor.to(DEV), fam.critic.to(DEV), fam.obs, fam.acts, logp, fam.rtg, fam.adv, F32(var))
            fam.actor.cpu(), fam.critic.cpu()
        else:
            ratio = torch.exp(lp - logp.cpu().double())   # (of the rounded log-probabilities the kernel reads)
            bad = (((ratio - 0.8).abs() < 2e-5) | ((ratio - 1.2).abs() < 2e-5)).to(DEV)
            if bool(bad.any()):
                good = int((~bad).nonzero()[0])
                for t in (fam.obs, fam.acts, logp, fam.rtg, fam.adv):
                    t[bad] = t[good].clone()
    fam._oa = None   # (x3: the rows are split again)
    return logp


@pytest.mark.parametrize("kind,D,f16,n", gc.FAMILIES, ids=gc.fam_ids)
def test_dlogvar_against_float64_within_the_allowance_of_float32_autograd(kind, D, f16, n):
    """var_state[4] at max_norm = +inf (coefficient 1) against float64 autograd; the error pooled over 8 seeds (root sum of squares)
    must not exceed 2.5 x that of PyTorch float32 autograd on the same batches -- the per-tensor allowance tests/test_gpu_bf16x3.py
    grants the split products."""
    var = 0.6
    for ent_coef in (0.0, 0.01):
        e_dev, e_t32 = [], []
        for seed in range(8):
            fam = VFamily(kind, D, f16, n, seed=20 + seed)
            logp = _kink_free_batch(fam, var, seed)
            obs64 = fam.obs.double()   # (float16 rows: the values the kernel widens)
            g64, ratio, clipped = _theta_grad(fam.actor, obs64, fam.acts, logp, fam.adv, F32(var), F32(ent_coef), torch.float64)
            share = float(clipped.double().mean())
            assert 0.05 <= share <= 0.95, f"clipped share {share}: both kinds of samples must be present"
            g32, _, _ = _theta_grad(fam.actor, fam.obs, fam.acts, logp, fam.adv, F32(var), F32(ent_coef), torch.float32)
            s, vs = fam.start(), vstate(var)
            fam.epoch_var(s, 1, vs, INF, _cs(), ent_coef=ent_coef, logp=logp)
            torch.cuda.synchronize()
            st = vs.tolist()
            assert st[STEPS] == 1.0
            e_dev.append(st[GRAD] - g64)
            e_t32.append(g32 - g64)
        pd, pt = math.sqrt(sum(e * e for e in e_dev)), math.sqrt(sum(e * e for e in e_t32))
        print(f"dlogvar {kind}-d{D}-{'f16' if f16 else 'f32'}-n{n} ent_coef={ent_coef}: pooled error device {pd:.3e}, torch float32 {pt:.3e}, "
              f"ratio {pd / pt:.3f} (|gradient| ~ {abs(g64):.3e})")
        assert pd <= 2.5 * pt, (pd, pt, pd / pt)


# ================================================================================================ 3: queued run against the host replay
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("kind,D,f16,n", gc.FAMILIES, ids=gc.fam_ids)
@pytest.mark.parametrize("adaptive", [False, True], ids=["constant_lr", "adaptive_lr"])
def test_eight_queued_calls_against_the_host_replay(kind, D, f16, n, adaptive):
    fam = VFamily(kind, D, f16, n)
    K, lr, ent = 8, 3e-3, 0.01
    s, vs = fam.start(), vstate(0.6)
    stats = torch.zeros((K, 8), device=DEV)
    cs = torch.full((K, 4), -7.0, device=DEV)
    snap = torch.zeros((K, 8), device=DEV)
    lr_state = torch.zeros(4, device=DEV) if adaptive else None
    lr_snap = torch.zeros((K, 4), device=DEV)
    for i in range(K):   # queued: nothing below waits for the device
        s["st"] = stats[i]
        fam.epoch_var(s, i + 1, vs, 0.5, cs[i], lr_state, adapt=int(i > 0), lr=lr, ent_coef=ent)
        snap[i].copy_(vs)
        if adaptive:
            lr_snap[i].copy_(lr_state)
    torch.cuda.synchronize()
    state = ppo.var_state_init(0.6)
    for i in range(K):
        step = i + 1
        rate = float(lr_snap[i, (step + 1) & 1]) if adaptive else lr
        state = ppo.learned_var_reference(state, float(stats[i, 3]), float(cs[i, 2]), ent, rate, HYPER[1:3], HYPER[3], step, 1e-3, 1.0)
        dev = snap[i].tolist()
        for k in (THETA, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED, ENTROPY):
            assert dev[k] == state[k], (kind, i, k, dev[k], state[k])
        assert _ulps(dev[VAR], math.exp(float(dev[THETA]))) <= 8, (kind, i, dev[VAR], math.exp(dev[THETA]))
        state[VAR] = dev[VAR]
    assert snap[-1, STEPS] == K and snap[-1, THETA] != snap[0, THETA]
    if adaptive:
        assert len({float(v) for v in lr_snap[:, :2].reshape(-1) if v != 0}) > 1, "the rate never moved: the adaptive leg shows nothing"


# ================================================================================================ 4: exact corners
@pytest.mark.parametrize("kind,D,f16,n", gc.FAMILIES, ids=gc.fam_ids)
def test_exact_corners(kind, D, f16, n):
    fam = VFamily(kind, D, f16, n)
    c = 0.01
    # all advantages zero: the gradient is exactly -ent_coef
    s, vs = fam.start(), vstate(0.6)
    fam.epoch_var(s, 1, vs, INF, _cs(), ent_coef=c, adv=torch.zeros_like(fam.adv))
    torch.cuda.synchronize()
    assert float(vs[GRAD]) == -F32(c) and float(vs[STEPS]) == 1.0 and float(vs[THETA]) > F32(math.log(F32(0.6)))
    # theta pinned at the upper clamp: the entropy bonus alone pushes the variance up
    s, vs = fam.start(), vstate(0.6)
    fam.epoch_var(s, 1, vs, INF, _cs(), ent_coef=c, var_min=0.5, var_max=0.6, adv=torch.zeros_like(fam.adv))
    torch.cuda.synchronize()
    assert float(vs[THETA]) == ppo.var_state_init(0.6)[THETA] and float(vs[STEPS]) == 1.0 and float(vs[ADAM_M]) != 0.0
    # ... and at both clamps by the loss alone.  With logp_old the policy's own log-probability every ratio is 1 (inside the clip
    # range) and d/d theta = -(1 / n) sum_i A_i h_i, h_i = 1/2 (d0^2 + d1^2)_i / var - 1: the advantages A = -h push the variance down,
    # A = +h push it up
    a64 = copy.deepcopy(fam.actor).cpu().double()
    with torch.no_grad():
        q = ((fam.acts.cpu().double() - a64(fam.obs.cpu().double())) ** 2).sum(-1) / F32(0.6)
        own_logp = (-0.5 * q - LOG_2PI - math.log(F32(0.6))).float().to(DEV).contiguous()
        h = (0.5 * q - 1.0).float().to(DEV).contiguous()
    for sign, bounds in ((-1.0, dict(var_min=0.6, var_max=1.0)), (1.0, dict(var_min=0.5, var_max=0.6))):
        free, pinned = vstate(0.6), vstate(0.6)
        fam.epoch_var(fam.start(), 1, free, INF, _cs(), adv=h * sign, logp=own_logp)
        fam.epoch_var(fam.start(), 1, pinned, INF, _cs(), adv=h * sign, logp=own_logp, **bounds)
        torch.cuda.synchronize()
        fr, pn = free.tolist(), pinned.tolist()
        assert fr[GRAD] * sign < 0 and (fr[THETA] - ppo.var_state_init(0.6)[THETA]) * sign > 0, (sign, fr)   # unclamped, theta moves
        assert pn[THETA] == ppo.var_state_init(0.6)[THETA] and pn[2:6] == fr[2:6], (sign, pn, fr)            # clamped, it stays; Adam's state moves
        assert _ulps(pn[VAR], math.exp(pn[THETA])) <= 8
    # a NaN advantage (of a sample whose ratio lies inside the clip range: outside it the clipped branch would hide the NaN): the
    # actor's coefficient is 0, theta, m and v are untouched, the skip is counted
    adv = fam.adv.clone()
    adv[n // 2] = float("nan")
    s, vs = fam.start(used=True), vstate(0.6)
    vs[ADAM_M], vs[ADAM_V] = 0.25, 0.125
    before, cs = vs.clone(), _cs()
    fam.epoch_var(s, 3, vs, 0.5, cs, ent_coef=c, adv=adv, logp=own_logp)
    torch.cuda.synchronize()
    assert float(cs[2]) == 0.0 and float(cs[3]) > 0.0
    assert torch.equal(vs[:6], before[:6]) and float(vs[SKIPPED]) == 1.0 and float(vs[ENTROPY]) == 0.0
    assert torch.equal(s["p"][:fam.PA], fam.flat[:fam.PA]) and not torch.equal(s["p"][fam.PA:], fam.flat[fam.PA:])
    # two calls on the same inputs give the same bits
    runs = []
    for _ in range(2):
        s, vs, cs = fam.start(used=True), vstate(FULL_MANTISSA), _cs()
        fam.epoch_var(s, 2, vs, 0.5, cs, ent_coef=c)
        torch.cuda.synchronize()
        runs.append((s, vs, cs))
    assert gc._same(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][0]["st"][:5], runs[1][0]["st"][:5])


# ================================================================================================ the batch tails, guarded
TAILS = [("mlp64", 16, 0, 1), ("mlp64", 16, 0, 77), ("mlp64", 42, 1, 77), ("x3", 16, 0, 1), ("x3", 16, 0, 77), ("x3", 42, 0, 77),
         ("resmlp", 16, 0, 1), ("resmlp", 16, 0, 33)]


@pytest.mark.parametrize("kind,D,f16,n", TAILS, ids=[f"{k}-d{d}-{'f16' if h else 'f32'}-n{n}" for k, d, h, n in TAILS])
def test_tails_inside_guarded_allocations(kind, D, f16, n):
    """n = 1 and a ragged tile inside guarded allocations, the state inside a guard of its own, at 256 bytes and at the ABI's minimum
    alignments: the guards hold, both placements give the same bits, the nets' step is the clipped epoch's and theta's the mirror's."""
    fam = VFamily(kind, D, f16, n)
    L, pre = fam.L, PREFIX[kind]
    oa = 16 if D == 16 else (4 if f16 else 8)
    wsb = L.navppo_resmlp512_workspace_bytes(n) if kind == "resmlp" else L.navppo_mlp64_workspace_bytes(D)
    var = FULL_MANTISSA
    written = torch.tensor([1, 1, 1, 1, 1, 0, 0, 0], dtype=torch.bool)

    def call(g):
        o = g.inp(fam.obs, oa)
        ac, lp, rt, ad = g.inp(fam.acts, 8), g.inp(fam.logp, 4), g.inp(fam.rtg, 4), g.inp(fam.adv, 4)
        if kind == "x3":
            prep = g.out((L.navppo_mlp64_bf16x3_prep_bytes(n, D),), torch.uint8, 16, written=torch.zeros(1, dtype=torch.bool))
            _ok(L.navppo_mlp64_bf16x3_prepare(P(o), D, f16, n, P(prep), _st()), "prepare")
            oargs = (P(prep), D)
        else:
            oargs = (P(o), f16) if kind == "resmlp" else (P(o), D, f16)
        out = {}
        for twin in ("clipped", "var"):
            pw, mw, vw = g.io(fam.flat, 16), g.io(fam.m0, 4), g.io(fam.v0, 4)
            gr = g.out((fam.PT,), torch.float32, 4)
            st = g.out((8,), torch.float32, 4, written=written if twin == "var" else written & torch.tensor([1, 1, 1, 0, 1, 0, 0, 0], dtype=torch.bool))
            cs = g.out((4,), torch.float32, 4)
            ws = g.scratch(wsb + 16, 256)
            head = (P(pw), *oargs, P(ac), P(lp), P(rt), P(ad), n)
            mid = (0.2, *HYPER, 2, P(mw), P(vw), P(gr), P(st), P(ws), 0.5, P(cs))
            if twin == "clipped":
                _ok(getattr(L, pre + "update_epoch_clipped")(*head, var, *mid, _st()), "clipped")
                out[twin] = (pw, mw, vw, gr, cs, st)
            else:
                vs = g.io(vstate(var), 16)
                _ok(getattr(L, pre + "update_epoch_var")(*head, *mid, *LR_ARGS, 0, None, 0.01, 1e-3, 1.0, P(vs), _st()), "var")
                out[twin] = (pw, mw, vw, gr, cs, st, vs)
        return out

    res = run_both(DEV, call, f"{kind} D={D} f16={f16} n={n}")
    a, b = res["clipped"], res["var"]
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    assert torch.equal(a[5][[0, 1, 2, 4]], b[5][[0, 1, 2, 4]])
    ref = ppo.learned_var_reference(ppo.var_state_init(var), float(b[5][3]), float(b[4][2]), 0.01, HYPER[0], HYPER[1:3], HYPER[3], 2, 1e-3, 1.0)
    dev = b[6].tolist()
    assert [dev[k] for k in (THETA, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED, ENTROPY)] == [ref[k] for k in (THETA, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED, ENTROPY)]
    assert _ulps(dev[VAR], math.exp(dev[THETA])) <= 8


# ================================================================================================ 5: every refusal
@pytest.mark.parametrize("kind,D,f16,n", [gc.FAMILIES[0], gc.FAMILIES[3], gc.FAMILIES[6]], ids=["mlp64", "x3", "resmlp"])
def test_every_refusal_of_the_entry_points(kind, D, f16, n):
    fam = VFamily(kind, D, f16, n)
    L = fam.L
    s, cs = fam.start(), _cs()
    before = {k: v.clone() for k, v in s.items()}
    nan = float("nan")

    def call(vs=None, null_state=False, ent_coef=0.0, var_min=1e-3, var_max=1.0, max_norm=0.5, cs_=cs, lr_state=None, lr_args=LR_ARGS, adapt=0,
             step=1, offset=0):
        vs = vstate(0.6) if vs is None else vs
        ptr = None if null_state else C.c_void_p(vs.data_ptr() + offset)
        rc = getattr(L, fam.prefix + "update_epoch_var")(P(s["p"]), *fam.oargs(), P(fam.acts), P(fam.logp), P(fam.rtg), P(fam.adv), fam.n, 0.2,
                                                         *HYPER, step, P(s["m"]), P(s["v"]), P(s["g"]), P(s["st"]), P(fam.ws), max_norm, P(cs_),
                                                         *lr_args, adapt, P(lr_state), ent_coef, var_min, var_max, ptr, _st())
        return rc, L.navppo_last_error()

    lrs = torch.zeros(4, device=DEV)
    bad = [dict(null_state=True), dict(offset=4), dict(offset=8), dict(ent_coef=-1e-9), dict(ent_coef=nan), dict(ent_coef=INF),
           dict(var_min=0.0), dict(var_min=-1.0), dict(var_min=nan), dict(var_max=nan), dict(var_max=INF), dict(var_min=0.5, var_max=0.25)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and b"var_state_dev" in msg, (kw, rc, msg)
    # what *_clipped / *_lr refuse
    for kw, word in ((dict(max_norm=0.0), b"max_norm"), (dict(max_norm=nan), b"max_norm"), (dict(cs_=None), b"clip_stats_dev"),
                     (dict(step=0), b"step"), (dict(lr_state=lrs, lr_args=(0.0, 1e-5, 1e-2)), b"kl_target"),
                     (dict(lr_state=lrs, lr_args=(0.01, 1e-2, 1e-5)), b"lr_min"), (dict(lr_state=lrs, adapt=2), b"adapt")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(s[k], before[k]) for k in s), "a refused call launched something"
    rc, msg = call(max_norm=INF, lr_state=None, lr_args=(nan, nan, nan), adapt=7)   # lr_state_dev NULL: the rule's arguments are not read
    assert rc == 0, msg


# ================================================================================================ 6: the trainer
def _env(n_envs, seed):
    from navbot_ppo_amd.env import VecEnv
    return VecEnv(n_envs, map="stage_1", max_episode_steps=30, seed=seed, device="cuda:0")




@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
@pytest.mark.parametrize("minibatch_size", [None, 512])
@pytest.mark.parametrize("lr_schedule", [None, "adaptive"])
def test_trainer_logs_the_mirrors_variance_and_rolls_out_with_it(policy, minibatch_size, lr_schedule, tmp_path):
    from navbot_ppo_amd import train_log
    T, N, n_ep = 32, 64, 3
    K = 1 if minibatch_size is None else -(-T * N // minibatch_size)
    env = _env(N, 5)
    cfg = ppo.PPOConfig(rollout_len=T, max_episode_steps=30, n_updates_per_iteration=n_ep, policy=policy, seed=2, learn_var=True, ent_coef=0.01,
                        minibatch_size=minibatch_size, minibatch_shuffle="none", lr_schedule=lr_schedule, lr=3e-3, max_grad_norm=0.5,
                        output_dir=str(tmp_path), save_freq=2)
    tr = ppo.PPOTrainer(env, cfg)
    up, D = tr.updater, tr.net_dim
    assert up.fused and tr.var.data_ptr() == up.var_state.data_ptr() + 4

    def stored_logp_under(flat, var):
        """gaussian_log_prob of the stored actions under the actor `flat` and the variance `var`, on the rollout's stored rows"""
        now = up.fp.flat.clone()
        up.fp.flat.copy_(flat)
        with torch.no_grad():
            lp = ppo.gaussian_log_prob(tr.actor(tr.net_obs[:T].reshape(T * N, D).float()), tr.act_buf.reshape(T * N, 2), torch.tensor(var, device=DEV))
        up.fp.flat.copy_(now)
        return lp.cpu().numpy()

    state, t, rate = ppo.var_state_init(cfg.init_var), 0, cfg.lr
    for it in range(4):
        var_before, flat_before = float(up.var_state[VAR]), up.fp.flat.clone()
        lg = tr.iteration()
        # this iteration's rollout drew its noise with the variance the last update ended on
        assert lg["rollout_var"] == var_before
        np.testing.assert_allclose(tr.logp_buf.reshape(-1).cpu().numpy(), stored_logp_under(flat_before, var_before), rtol=1e-4, atol=3e-5)
        # the mirror replays the update's steps from the recorded sums, coefficients and (adaptive) approx_kl
        rows, css = up._fhist[:n_ep * K].tolist(), up.clip_stats[:n_ep * K].tolist()
        for i in range(n_ep * K):
            t += 1
            if lr_schedule == "adaptive":
                rate = ppo.adaptive_lr_reference(rate, rows[i][1], cfg.desired_kl, cfg.lr_min, cfg.lr_max, adapt=i > 0)
            state = ppo.learned_var_reference(state, rows[i][3], css[i][2], cfg.ent_coef, rate, ppo.ADAM_HYPER[:2], ppo.ADAM_HYPER[2], t,
                                              cfg.var_min, cfg.var_max)
        dev = up.var_state.tolist()
        assert [dev[k] for k in (THETA, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED)] == [state[k] for k in (THETA, ADAM_M, ADAM_V, GRAD, STEPS, SKIPPED)], it
        state[VAR] = dev[VAR]
        assert lg["var"] == dev[VAR] and lg["std"] == math.sqrt(dev[VAR]) and lg["var_steps_skipped"] == 0 and lg["var_grad"] == dev[GRAD]
        assert lg["entropy"] == pytest.approx(1.0 + LOG_2PI + dev[THETA], abs=1e-12)
        assert " var_grad=" in train_log.progress_line(lg) and train_log.tb_scalars(lg, cfg)["ppo/var"] == dev[VAR]
    assert dev[STEPS] == 4 * n_ep * K
    # ... and the variance moved far enough for the log-probability check to tell it from the start value
    tr.rollout()
    got = tr.logp_buf.reshape(-1).cpu().numpy()
    np.testing.assert_allclose(got, stored_logp_under(up.fp.flat, dev[VAR]), rtol=1e-4, atol=3e-5)
    assert np.abs(got - stored_logp_under(up.fp.flat, F32(cfg.init_var))).max() > 1e-3
    # a checkpoint round trip restores the state (iteration 4 saved one)
    ck = tr.checkpoint_dir()
    tag = "iter%04d_step%08d.pth" % (tr.i_so_far, tr.t_so_far)
    files = {kind: [f for f in os.listdir(ck) if f.endswith(tag) and kind in f] for kind in ("actor", "critic", "explore")}
    assert all(len(v) == 1 for v in files.values()), files
    env2 = _env(N, 5)
    tr2 = ppo.PPOTrainer(env2, cfg)
    tr2.load_checkpoint(os.path.join(ck, files["actor"][0]), os.path.join(ck, files["critic"][0]))
    d2 = tr2.updater.var_state.tolist()
    assert [d2[k] for k in (THETA, ADAM_M, ADAM_V, STEPS)] == [dev[k] for k in (THETA, ADAM_M, ADAM_V, STEPS)]
    assert _ulps(d2[VAR], dev[VAR]) <= 8 and float(tr2.var) == d2[VAR]
    env.close()
    env2.close()
