"""The four twins of the fused update (navppo_*_update_epoch_clipped, _kl, _lr, _var) at the launch geometries the other twin tests never
reach, and d/d(log var) per sample against float64.

tests/test_gpu_grad_clip.py, test_gpu_target_kl.py, test_gpu_adaptive_lr.py and test_gpu_learned_var.py run at n <= 8229: every wave of a
2x64 pass owns one tile, every reduction runs its remainder loop only, var_step_kernel adds at most 258 rows and no grid is capped.
tests/test_gpu_tails.py goes wide with float64 probes, but calls *_loss_grad and the unclipped *_update_epoch only.  WIDE below holds the
smallest batches at which each mechanism first engages; the expected grid and row counts stand beside each shape as plain numbers and are
asserted from the launch plans' formulas (_geometry), so a moved cap fails the test instead of silently ending its coverage.

  1. At WIDE, from a used optimiser state, two steps, max_norm = +inf and a bound that clips both nets: the gradient output of
     *_update_epoch is *_loss_grad's bit for bit (which carries test_gpu_tails' float64 probes over to the epochs); *_clipped(+inf) is
     *_update_epoch; *_clipped(finite) against float64 (the bounds of test_gpu_grad_clip, unchanged); *_kl(+inf), *_lr (adapt = 0, and
     lr_min == lr_max == lr) and *_var (the state's variance by value, lr_state NULL and given) are *_clipped bit for bit; a tripped
     *_kl gate stays shut on capped grids.  The workspace is filled with NaN before EVERY call: it is scratch, and a reduction or a
     var_step_kernel that read a row nobody wrote would turn finite results into NaN.
  2. d/d(log var) of *_update_epoch_var on probe batches (every non-probe position carries one row with adv = 0, whose term is exactly
     0 on both sides) against float64 autograd, within a quarter of the smallest carrying probe's share: a CONDITION, not a measurement
     -- a probe dropped, counted twice, read from the wrong row or left unmasked breaks it by a factor of 4 at least.  Regime A: every
     probe carries, none below a tenth of the largest; regime B: every other probe lies outside the clip range on the side where the
     clipped branch is the minimum (its term is exactly 0).

The precondition of 2 -- PyTorch float32 autograd on the same probe batches stays below a tenth of that bound -- is asserted on the CPU
by tests/test_twins_wide_cpu.py for every shape and both regimes (worst ratio of float32 error to bound measured there: 2.7e-5, so the
tenth is met with a factor of 3000 to spare; profiles/twins_wide.txt has the figures per case).  The device-to-float32 error ratio is
printed, not asserted: the 2.5 x accuracy gate lives in test_gpu_learned_var.py, this module is about geometry."""
import copy
import math

import numpy as np
import pytest
import torch

from _guards import Guards
from navbot_ppo_amd import ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.explore_var import ADAM_M, ADAM_V, GRAD, SKIPPED, STEPS, THETA, VAR
from test_gpu_adaptive_lr import LR0, LrFamily
from test_gpu_grad_clip import DEV, F32, HYPER, INF, U, Family, P, _check_adam, _check_clip, _ok, _same, _st
from test_gpu_learned_var import FULL_MANTISSA, LR_ARGS, PREFIX, VFamily, _theta_grad, vstate
from test_gpu_tails import MLP64_N, RES_N, _leaky_kinks, _mlp64_flat, _obs_align, _probe_positions, _relu_kinks, _resmlp_flat, _tile_probes
from test_gpu_target_kl import KLFamily

pytestmark = pytest.mark.gpu
NAN = float("nan")
CLIP = 0.2
assert issubclass(LrFamily, KLFamily) and issubclass(KLFamily, Family)   # (logp_old of an LrFamily: the start policy's own)


# ================================================================================================ the shapes
def _geometry(kind, D, n):
    """What the launch plans give at n samples (csrc/ppo_mlp64.hip plan_pass, csrc/ppo_resmlp512.hip make_plan; the constants are named
    in tests/test_gpu_tails.py _probe_positions): workgroups, the most tiles a wave takes, rows per reduction, trips of the reductions'
    unrolled loop (four rows per trip and row group, kRedGroups = 16 groups: a trip while b + 48 < rows) and rows left to their
    remainder loop for row group 0, rows and trips (256 threads) of var_step_kernel."""
    tiles = (n + 31) // 32

    def red(rows):   # row group 0 of reduce_adam / resmlp_reduce: (unrolled trips, remainder rows)
        b = trips = 0
        while b + 48 < rows:
            b, trips = b + 64, trips + 1
        return trips, len(range(b, rows, 16))

    if kind == "resmlp":
        g = min((tiles + 7) // 8, 256 // (4 * 2))          # groups: kMaxWG / (NSL x 2 nets) = 32 at the most
        if g >= 8:
            g &= ~7
        e_blocks = min(tiles, 1024)                         # resmlp_e2: 32 samples per workgroup and trip, kEMaxBlocks = 1024
        return dict(wgs=g * 4 * 2, groups=g, tiles_per_wave=-(-tiles // (g * 8)), e_blocks=e_blocks, e2_trips=-(-n * 8 // (e_blocks * 256)),
                    reduce_rows=(g * 8, g * 4, e_blocks), reduce_loops=(red(g * 8), red(g * 4), red(e_blocks)), var_rows=e_blocks,
                    var_trips=-(-e_blocks // 256))
    wgs = min((tiles + 7) // 8, 256)                        # kWWaves = 8 tiles per workgroup wanted, kWMaxBlocks = 256
    waves = 8 if (kind, D) == ("mlp64", 16) else 4          # Pad<16>::NW = 8; MLP64_WIDE_WAVES, x3s::SW, XPad<42>::NW = 4
    stride = wgs * waves
    return dict(wgs=wgs, waves=waves, tiles_per_wave=-(-tiles // stride), waves_on_the_last_trip=tiles - (-(-tiles // stride) - 1) * stride,
                reduce_rows=wgs, reduce_loops=red(wgs), var_rows=wgs, var_trips=-(-wgs // 256))


N67 = 32 * 8 * 67 - 5   # 17147
# (kind, D, f16, n, what the plans give there)
WIDE = [
    # 536 tiles on 67 workgroups of 8 waves: not capped, one tile per wave, ragged; reduce_adam's unrolled loop runs once (rows 0 .. 63)
    # and leaves rows 64 .. 66 to the remainder (one row for row group 0)
    ("mlp64", 16, 0, N67, dict(wgs=67, waves=8, tiles_per_wave=1, waves_on_the_last_trip=536, reduce_rows=67, reduce_loops=(1, 1), var_rows=67,
                               var_trips=1)),
    # 2050 tiles on the cap of 256 workgroups x 8 waves = 2048: two waves take a second tile, the last one ragged (33 rows past 65536)
    ("mlp64", 16, 0, MLP64_N[2], dict(wgs=256, waves=8, tiles_per_wave=2, waves_on_the_last_trip=2, reduce_rows=256, reduce_loops=(4, 0),
                                      var_rows=256, var_trips=1)),
    ("mlp64", 16, 1, MLP64_N[2], dict(wgs=256, waves=8, tiles_per_wave=2, waves_on_the_last_trip=2, reduce_rows=256, reduce_loops=(4, 0),
                                      var_rows=256, var_trips=1)),
    # 2049 tiles on 256 x 4 waves = 1024: the tile loop wraps twice, one wave takes a third (ragged) tile
    ("mlp64", 42, 0, MLP64_N[3], dict(wgs=256, waves=4, tiles_per_wave=3, waves_on_the_last_trip=1, reduce_rows=256, reduce_loops=(4, 0),
                                      var_rows=256, var_trips=1)),
    ("x3", 16, 0, MLP64_N[3], dict(wgs=256, waves=4, tiles_per_wave=3, waves_on_the_last_trip=1, reduce_rows=256, reduce_loops=(4, 0),
                                   var_rows=256, var_trips=1)),
    ("x3", 42, 0, MLP64_N[3], dict(wgs=256, waves=4, tiles_per_wave=3, waves_on_the_last_trip=1, reduce_rows=256, reduce_loops=(4, 0),
                                   var_rows=256, var_trips=1)),
    # 257 tiles: 33 groups wanted, 32 (the cap) launched, so the 8-wave kernels wrap; 257 rows of resmlp_e2: var_step_kernel's second
    # trip carries exactly one row, resmlp_reduce's unrolled loop runs four times on them and leaves one row to group 0's remainder
    ("resmlp", 16, 0, RES_N[2], dict(wgs=256, groups=32, tiles_per_wave=2, e_blocks=257, e2_trips=1, reduce_rows=(256, 128, 257),
                                     reduce_loops=((4, 0), (2, 0), (4, 1)), var_rows=257, var_trips=2)),
    # 1563 tiles: resmlp_e2 capped at 1024 workgroups strides over the samples (a second trip for 539 of them); var_step_kernel takes
    # four trips; the 8-wave kernels take up to seven tiles per wave
    ("resmlp", 16, 0, RES_N[3], dict(wgs=256, groups=32, tiles_per_wave=7, e_blocks=1024, e2_trips=2, reduce_rows=(256, 128, 1024),
                                     reduce_loops=((4, 0), (2, 0), (16, 0)), var_rows=1024, var_trips=4)),
]
wide_ids = [f"{k}-d{d}-{'f16' if h else 'f32'}-n{n}" for k, d, h, n, _ in WIDE]
SHAPES = [w[:4] for w in WIDE]
STICKY = [SHAPES[1], SHAPES[4], SHAPES[7]]   # the two capped 2x64 shapes of the issue (65569 f32, 65541 x3 D16) and resmlp at 50001
assert (N67, MLP64_N[2], MLP64_N[3], RES_N[2], RES_N[3]) == (17147, 65569, 65541, 8209, 50001)


def test_the_shapes_reach_what_they_are_here_for():
    for kind, D, f16, n, want in WIDE:
        assert _geometry(kind, D, n) == want, (kind, D, n, _geometry(kind, D, n))
    # ... and one sample less than each cap's threshold does not reach it: the shapes are the smallest
    assert _geometry("mlp64", 16, 65536)["tiles_per_wave"] == 1 and _geometry("mlp64", 42, 65536)["tiles_per_wave"] == 2
    assert _geometry("mlp64", 16, 32 * 48)["reduce_loops"][0] == 0 and _geometry("resmlp", 16, 8192)["var_trips"] == 1
    assert _geometry("resmlp", 16, 32 * 1024)["e2_trips"] == 1 and _geometry("resmlp", 16, 32 * 1024 + 1)["e2_trips"] == 2


# ================================================================================================ 1: the twins are the base epoch
_fams = {}
KEYS = ("p", "m", "v", "g")
ST = [0, 1, 2, 4]


def _nan_ws(fam):
    fam.ws.fill_(NAN)


def _snap(s, keys=KEYS + ("st", "cs")):
    return {k: s[k].clone() for k in keys}


def _family(kind, D, f16, n):
    """Per shape, built once and left unchanged: the LrFamily (base, *_clipped, *_kl, *_lr; logp_old the start policy's own), the VFamily
    (*_var against *_clipped; the random logp_old of Family), the bound that clips both nets of each, and the reference runs on the
    LrFamily: two *_clipped steps from the used state per max_norm, with each step's state before, unclipped gradient and state after."""
    key = (kind, D, f16, n)
    if key not in _fams:
        fam, vfam = LrFamily(kind, D, f16, n), VFamily(kind, D, f16, n)
        _nan_ws(fam)
        norms = [float(g.double().norm()) for g in fam.nets_of(fam.loss_grad(fam.flat))]
        # (the VFamily's epochs run at the variance FULL_MANTISSA, *_loss_grad of Family at 0.6: its norms from a *_clipped(+inf) call)
        cs = torch.full((4,), -7.0, device=DEV)
        _nan_ws(vfam)
        vfam.epoch(vfam.start(used=True), 1, FULL_MANTISSA, INF, cs)
        vnorms = cs[:2].double().sqrt().tolist()
        assert all(x > 0 and math.isfinite(x) for x in norms + vnorms), (norms, vnorms)
        bounds = [F32(0.5 * min(norms)), F32(0.5 * min(vnorms))]
        runs = {}
        for mn in (INF, bounds[0]):
            s, steps = fam.start(used=True), []
            for step in (1, 2):
                before = _snap(s, ("p", "m", "v"))
                _nan_ws(fam)
                gu = fam.loss_grad(s["p"])
                _nan_ws(fam)
                fam.epoch_clipped(s, step, LR0, mn)
                steps.append(dict(before=before, gu=gu, after=_snap(s)))
            runs[mn] = steps
        _fams[key] = dict(fam=fam, vfam=vfam, bound=bounds[0], vbound=bounds[1], runs=runs)
    return _fams[key]


def _is_the_clipped(s, ref, what):
    assert _same(s, ref), what
    assert torch.equal(s["st"][ST], ref["st"][ST]) and torch.equal(s["cs"], ref["cs"]), what
    assert bool(torch.isfinite(s["p"]).all()) and bool(torch.isfinite(s["g"]).all()), what


@pytest.mark.parametrize("kind,D,f16,n", SHAPES, ids=wide_ids)
def test_gradient_is_loss_grads_and_clipped_is_the_base_epoch_or_float64s(kind, D, f16, n):
    F = _family(kind, D, f16, n)
    fam, PA = F["fam"], F["fam"].PA
    # the base epoch's gradient output is *_loss_grad's, at the weights of every reference step (both bounds: four sets of weights)
    for mn, steps in F["runs"].items():
        for step, r in enumerate(steps, 1):
            b = dict({k: r["before"][k].clone() for k in ("p", "m", "v")}, g=torch.zeros_like(fam.flat), st=torch.zeros(8, device=DEV))
            _nan_ws(fam)
            fam.epoch(b, step)
            assert torch.equal(b["g"], r["gu"]), (mn, step)
            assert bool(torch.isfinite(b["g"]).all()) and not torch.equal(b["p"], r["before"]["p"])
            if mn == INF:   # *_clipped(+inf) is this epoch; the coefficients are exactly 1
                a = r["after"]
                assert _same(a, b), step
                assert torch.equal(a["st"][ST], b["st"][ST]) and a["cs"][2:].tolist() == [1.0, 1.0], (step, a["cs"])
    assert not torch.equal(F["runs"][INF][0]["after"]["p"], F["runs"][INF][1]["after"]["p"])
    # *_clipped(finite) against float64 on that step's unclipped gradient
    mn = F["bound"]
    for step, r in enumerate(F["runs"][mn], 1):
        a, what = r["after"], f"{kind} d{D} n{n} step {step}"
        coefs = _check_clip(fam, r["gu"], a["cs"], mn, what)
        if step == 1:
            assert coefs[0] < 1.0 and coefs[1] < 1.0, coefs
        for k, (gk, gd) in enumerate(zip(fam.nets_of(r["gu"]), fam.nets_of(a["g"]))):
            want = gk.double() * float(a["cs"][2 + k])   # the kernel's own float32 coefficient
            assert bool(((gd.double() - want).abs() <= 2 * (2 * U) * want.abs() + 2.0 ** -140).all()), (what, k)
        _check_adam(r["before"]["p"], r["before"]["m"], r["before"]["v"], a["g"], step, a["p"], a["m"], a["v"], what=what)


@pytest.mark.parametrize("kind,D,f16,n", SHAPES, ids=wide_ids)
def test_kl_with_an_infinite_limit_is_the_clipped_epoch(kind, D, f16, n):
    F = _family(kind, D, f16, n)
    fam = F["fam"]
    for mn, steps in F["runs"].items():
        s = fam.start(used=True)
        for step, r in enumerate(steps, 1):
            _nan_ws(fam)
            fam.epoch_kl(s, step, INF, mn)
            _is_the_clipped(s, r["after"], (mn, step))
        assert s["kl"].tolist() == [0.0, 2.0, 0.0, 0.0]


@pytest.mark.parametrize("kind,D,f16,n", SHAPES, ids=wide_ids)
def test_lr_with_the_rate_held_is_the_clipped_epoch(kind, D, f16, n):
    """adapt = 0, and adapt = 1 between clamps that pin the rate (lr_min == lr_max == lr)"""
    F = _family(kind, D, f16, n)
    fam = F["fam"]
    for mn, steps in F["runs"].items():
        for kw in (dict(adapt=0), dict(adapt=1, lr_min=LR0, lr_max=LR0)):
            s = fam.start(used=True)
            for step, r in enumerate(steps, 1):
                _nan_ws(fam)
                fam.epoch_lr(s, step, 0.01, max_norm=mn, **kw)
                _is_the_clipped(s, r["after"], (mn, kw, step))
            assert s["lr"][:2].tolist() == [LR0, LR0], (kw, s["lr"])


@pytest.mark.parametrize("kind,D,f16,n", SHAPES, ids=wide_ids)
def test_var_is_the_clipped_epoch_with_the_states_variance_by_value(kind, D, f16, n):
    """as test_gpu_learned_var.py's test_the_nets_step_is_the_clipped_epochs_bit_for_bit: lr_state NULL (against *_clipped) and given
    (against *_lr), the second step with the variance the first one left"""
    F = _family(kind, D, f16, n)
    fam = F["vfam"]
    for mn in (INF, F["vbound"]):
        for adaptive in (False, True):
            a, b, vs = fam.start(used=True), fam.start(used=True), vstate(FULL_MANTISSA)
            lra = torch.tensor([1e-3, 1e-3, 0, 0], device=DEV) if adaptive else None
            lrb = None if lra is None else lra.clone()
            for step in (1, 2):
                v_now = float(vs[VAR])
                assert step > 1 or v_now == FULL_MANTISSA
                ca, cb = torch.full((4,), -7.0, device=DEV), torch.full((4,), -7.0, device=DEV)
                _nan_ws(fam)
                fam.epoch(a, step, v_now, mn, ca, lra, adapt=int(step > 1))
                _nan_ws(fam)
                fam.epoch_var(b, step, vs, mn, cb, lrb, adapt=int(step > 1), ent_coef=0.01)
                torch.cuda.synchronize()
                what = f"{kind} d{D} n{n} max_norm={mn} adaptive={adaptive} step={step}"
                assert _same(a, b) and torch.equal(ca, cb) and torch.equal(a["st"][ST], b["st"][ST]), what
                assert bool(torch.isfinite(b["p"]).all()) and bool(torch.isfinite(b["g"]).all()) and math.isfinite(float(b["st"][3])), what
                if step == 1:
                    assert cb[2:].tolist() == [1.0, 1.0] if mn == INF else (float(cb[2]) < 1.0 and float(cb[3]) < 1.0), (what, cb)
                if adaptive:
                    assert torch.equal(lra, lrb), what
            st = vs.tolist()
            assert st[STEPS] == 2.0 and st[SKIPPED] == 0.0 and st[VAR] != FULL_MANTISSA and math.isfinite(st[VAR]), st


@pytest.mark.parametrize("kind,D,f16,n", STICKY, ids=[wide_ids[SHAPES.index(s)] for s in STICKY])
def test_a_tripped_gate_stays_shut_on_capped_grids(kind, D, f16, n):
    """kl_limit = half the approx_kl the tripping step measures, strictly between 0 and it; the gated call of that step trips (nothing
    is stepped); then, with the outputs filled with -7, two more calls return at every kernel's entry on all 256 workgroups (1024 of
    resmlp_e2).  The tripping step is the SECOND: at the start weights logp_old is the policy's own log-probability up to a few ulps,
    the log-ratio of a sample is 0 or a few units of 2^-22, exp of that is 1 + itself exactly, and approx_kl = mean((ratio - 1) -
    log ratio) is exactly 0 (measured: 0 on all three shapes) -- no limit lies strictly below it.  Step 1 therefore passes the gate
    (0 <= kl_limit) and must be the clipped epoch's; step 2, on the weights step 1 left, trips."""
    F = _family(kind, D, f16, n)
    fam, ref = F["fam"], F["runs"][INF]
    kl1, kl2 = float(ref[0]["after"]["st"][1]), float(ref[1]["after"]["st"][1])
    kl_limit = F32(0.5 * kl2)
    print(f"sticky {kind} d{D} n{n}: approx_kl of step 1 = {kl1:.9g}, of step 2 = {kl2:.9g}, kl_limit = {kl_limit:.9g}")
    assert kl1 <= kl_limit and 0.0 < kl_limit < kl2, (kl1, kl_limit, kl2)
    s = fam.start(used=True)
    _nan_ws(fam)
    fam.epoch_kl(s, 1, kl_limit)
    _is_the_clipped(s, ref[0]["after"], "step 1, below the limit")
    assert s["kl"].tolist() == [0.0, 1.0, 0.0, 0.0]
    _nan_ws(fam)
    fam.epoch_kl(s, 2, kl_limit)
    for k in ("p", "m", "v"):
        assert torch.equal(s[k], ref[0]["after"][k]), k
    assert s["kl"].tolist() == [1.0, 1.0, kl2, 2.0] and s["cs"][2:].tolist() == [0.0, 0.0]
    assert torch.equal(s["g"], ref[1]["gu"]) and torch.equal(s["st"][ST], ref[1]["after"]["st"][ST])   # the trip's own pass ran
    keep = _snap(s, ("p", "m", "v", "kl"))
    for step in (3, 4):
        for k in ("g", "st", "cs"):
            s[k].fill_(-7.0)
        _nan_ws(fam)
        fam.epoch_kl(s, step, kl_limit)
        for k in ("p", "m", "v", "kl"):
            assert torch.equal(s[k], keep[k]), (k, step)
        for k in ("g", "st", "cs"):
            assert bool((s[k] == -7.0).all()), (k, step)


# ================================================================================================ 2: d/d(log var) by probes
def _nets(kind, D, seed):
    """(actor, critic, flat) of tests/test_gpu_tails.py's probe cases, on that module's device"""
    return _resmlp_flat(seed % 7 + 1) if kind == "resmlp" else _mlp64_flat(D, seed % 7 + 1)


def _positions(kind, n, seed):
    pos = set(_probe_positions(n, "resmlp512" if kind == "resmlp" else "f32", seed).tolist())
    if kind == "resmlp":   # resmlp_e2 holds the sum: 32 samples per workgroup and trip, its grid capped at 1024
        pos |= _tile_probes(n, 1, min((n + 31) // 32, 1024))
    return np.array(sorted(p for p in pos if 0 <= p < n))


def _candidates(a64, c64, m, D, f16, gen, var64, kinks, lo, hi, eps=1e-4):
    """m candidate rows (CPU, float64 views of the values as stored) with ratio in [lo, hi], and which of them lie away from every unit's
    kink: obs, act, logp_old, rtg = V - (5 .. 15), |adv| in 0.5 .. 1.5, the ratio of the stored logp_old, h = 1/2 q / var - 1"""
    x = torch.rand((m, D), generator=gen, dtype=torch.float64)
    x = (x.half() if f16 else x.float()).double()
    act = torch.stack([torch.rand(m, generator=gen), torch.rand(m, generator=gen) * 2 - 1], 1)
    with torch.no_grad():
        mean = a64(x)
        lp = ppo.gaussian_log_prob(mean, act.double(), var64)
        r = lo + (hi - lo) * torch.rand(m, generator=gen, dtype=torch.float64)
        logp_old = (lp - torch.log(r)).float()
        ratio = torch.exp(lp - logp_old.double())
        V = c64(x).squeeze(-1)
        rtg = (V - 5.0 - 10.0 * torch.rand(m, generator=gen, dtype=torch.float64)).float()
        mag = (0.5 + torch.rand(m, generator=gen)).float()
        h = 0.5 * ((act.double() - mean) ** 2).sum(-1) / var64 - 1.0
        ok = ~(kinks(a64, x, eps) | kinks(c64, x, eps)) & (ratio >= lo) & (ratio <= hi)
    return dict(x=x, act=act, logp=logp_old, rtg=rtg, mag=mag, ratio=ratio, h=h, V=V), ok


def _take(c, idx):
    return {k: v[idx] for k, v in c.items()}


def _cat(cs):
    return {k: torch.cat([c[k] for c in cs]) for k in cs[0]}


def probe_batch(actor, critic, kind, D, f16, n, regime, seed, var=FULL_MANTISSA):
    """One probe batch on the CPU.  Regime "A": every probe's ratio in [0.85, 1.15] (its unclipped branch is live), and none with
    |t_i| = |adv_i ratio_i h_i| below a tenth of the largest.  Regime "B": every other probe (in position order) instead has its ratio
    in [1.3, 1.6] with adv > 0 or in [0.5, 0.7] with adv < 0, alternating: the clipped branch is the minimum, t_i = 0 exactly.  Every
    non-probe position carries one background row with adv = 0, logp_old its own log-probability and rtg its own value.
    Returns the batch (obs in its stored type) and pos, the probes' rows, t (float64, per probe; 0 where masked), carrying (mask)."""
    gen = torch.Generator().manual_seed(7919 * seed + (1 if regime == "B" else 0))
    a64, c64 = copy.deepcopy(actor).cpu().double(), copy.deepcopy(critic).cpu().double()
    kinks = _leaky_kinks if kind == "resmlp" else _relu_kinks
    var64 = torch.tensor(var, dtype=torch.float64)
    pos = torch.as_tensor(_positions(kind, n, seed))
    k = pos.numel()
    masked = (torch.arange(k) % 2 == 1) if regime == "B" else torch.zeros(k, dtype=torch.bool)
    kc, km = int((~masked).sum()), int(masked.sum())
    # the carrying probes: a pool that grows until kc of it reach a tenth of ITS largest |t| (so they reach a tenth of their own)
    pool = []
    while True:
        c, ok = _candidates(a64, c64, 4 * kc + 64, D, f16, gen, var64, kinks, 0.85, 1.15)
        pool.append(_take(c, ok.nonzero().squeeze(1)))
        allc = _cat(pool)
        tabs = (allc["mag"].double() * allc["ratio"] * allc["h"]).abs()
        keep = (tabs >= 0.1 * tabs.max()).nonzero().squeeze(1)
        if keep.numel() > kc:   # (one more than needed: the background row)
            break
    carry, bg = _take(allc, keep[:kc]), _take(allc, keep[kc:kc + 1])
    sign = (torch.randint(0, 2, (kc,), generator=gen) * 2 - 1).float()
    carry["adv"] = carry.pop("mag") * sign
    rows = {key: torch.empty((k,) + tuple(v.shape[1:]), dtype=v.dtype) for key, v in carry.items()}
    for key in rows:
        rows[key][~masked] = carry[key]
    if km:   # the masked probes: above the range with adv > 0, below it with adv < 0; the term each would add if the mask were not
        # applied is no smaller than the smallest carrying one's, so ONE of them left unmasked misses the bound by the same factor of 4
        floor = float((carry["adv"].double() * carry["ratio"] * carry["h"]).abs().min())
        parts = []
        for j, (lo, hi, sg) in enumerate(((1.3, 1.6, 1.0), (0.5, 0.7, -1.0))):
            need, got = (km + 1 - j) // 2, []
            while sum(g["x"].shape[0] for g in got) < need:
                c, ok = _candidates(a64, c64, 4 * need + 16, D, f16, gen, var64, kinks, lo, hi)
                ok &= (c["mag"].double() * c["ratio"] * c["h"]).abs() >= floor
                got.append(_take(c, ok.nonzero().squeeze(1)))
            part = _take(_cat(got), torch.arange(need))
            part["adv"] = part.pop("mag") * sg
            parts.append(part)
        inter = {key: torch.empty((km,) + tuple(v.shape[1:]), dtype=v.dtype) for key, v in parts[0].items()}
        for key in inter:
            inter[key][0::2], inter[key][1::2] = parts[0][key], parts[1][key]
        for key in rows:
            rows[key][masked] = inter[key]
    # t_i = dL_dlp_i n (1/2 q_i / var - 1), dL_dlp_i n = -adv_i ratio_i where the unclipped branch is live
    s1, s2 = rows["ratio"] * rows["adv"].double(), rows["ratio"].clamp(1 - CLIP, 1 + CLIP) * rows["adv"].double()
    carrying = ((rows["ratio"] >= 1 - CLIP) & (rows["ratio"] <= 1 + CLIP)) | (s1 < s2)
    assert torch.equal(carrying, ~masked), "the regimes' probes carry / are masked as drawn"
    t = torch.where(carrying, -rows["adv"].double() * rows["ratio"] * rows["h"], torch.zeros(k, dtype=torch.float64))
    assert float(t[carrying].abs().min()) >= 0.1 * float(t.abs().max()) > 0.0
    odt = torch.float16 if f16 else torch.float32
    with torch.no_grad():
        lp0 = ppo.gaussian_log_prob(a64(bg["x"]), bg["act"].double(), var64).float()
    obs = bg["x"].to(odt).expand(n, D).contiguous()
    acts, logp, rtg = bg["act"].expand(n, 2).contiguous(), lp0.expand(n).contiguous(), bg["V"].float().expand(n).contiguous()
    adv = torch.zeros(n)
    obs[pos], acts[pos], logp[pos], rtg[pos], adv[pos] = rows["x"].to(odt), rows["act"], rows["logp"], rows["rtg"], rows["adv"]
    return dict(obs=obs, acts=acts, logp=logp, rtg=rtg, adv=adv, pos=pos, rows=rows, t=t, carrying=carrying)


def probe_reference(actor, batch, n, var=FULL_MANTISSA):
    """float64 and float32 autograd of the surrogate over the probes with respect to theta = log var (test_gpu_learned_var._theta_grad),
    scaled by k / n (the background adds exactly 0); the bound: a quarter of the smallest carrying probe's share."""
    pos, rows, t = batch["pos"], batch["rows"], batch["t"]
    k = pos.numel()
    args = (batch["acts"][pos], batch["logp"][pos], batch["adv"][pos], F32(var), 0.0)
    g64, _, clipped = _theta_grad(actor, batch["obs"][pos].double(), *args, torch.float64)
    g32, _, _ = _theta_grad(actor, batch["obs"][pos], *args, torch.float32)
    assert torch.equal(~clipped, batch["carrying"])
    g64, g32 = g64 * k / n, g32 * k / n
    assert abs(g64 - float(t.sum()) / n) <= 1e-12 * float(t.abs().sum()) / n, (g64, float(t.sum()) / n)   # the closed form is autograd's
    bound = 0.25 * float(t[batch["carrying"]].abs().min()) / n
    assert bound >= 0.025 * float(t.abs().max()) / n * (1 - 1e-12)
    return g64, g32, bound


_pooled = {}


def _var_call(kind, D, f16, n, flat, b, adv, ent_coef, what):
    """*_update_epoch_var at step 1, max_norm = +inf, variance FULL_MANTISSA, every argument guarded at the ABI's minimum alignment (the
    state 16-byte), the workspace NaN inside its guards.  Returns (stats [8], clip_stats [4], var_state [8]) on the host."""
    L, pre = lib(), PREFIX[kind]
    gd = Guards(DEV, minimal=True)
    o = gd.inp(b["obs"], 16 if kind == "resmlp" else _obs_align(D, f16))
    ac, lp, rt, ad = gd.inp(b["acts"], 8), gd.inp(b["logp"], 4), gd.inp(b["rtg"], 4), gd.inp(adv, 4)
    if kind == "x3":
        prep = gd.out((L.navppo_mlp64_bf16x3_prep_bytes(n, D),), torch.uint8, 16, written=torch.zeros(1, dtype=torch.bool))
        _ok(L.navppo_mlp64_bf16x3_prepare(P(o), D, f16, n, P(prep), _st()), "prepare")
        oargs = (P(prep), D)
    else:
        oargs = (P(o), f16) if kind == "resmlp" else (P(o), D, f16)
    pw, mw, vw = gd.io(flat, 16), gd.io(torch.zeros_like(flat), 4), gd.io(torch.zeros_like(flat), 4)
    gr = gd.out(flat.shape, torch.float32, 4)
    st = gd.out((8,), torch.float32, 4, written=torch.tensor([1, 1, 1, 1, 1, 0, 0, 0], dtype=torch.bool))
    cs = gd.out((4,), torch.float32, 4)
    wsb = L.navppo_resmlp512_workspace_bytes(n) + 16 if kind == "resmlp" else L.navppo_mlp64_workspace_bytes(D)
    ws = gd.scratch(wsb, 256)
    ws.view(torch.float32).fill_(NAN)
    vs = gd.io(vstate(FULL_MANTISSA), 16)
    _ok(getattr(L, pre + "update_epoch_var")(P(pw), *oargs, P(ac), P(lp), P(rt), P(ad), n, CLIP, *HYPER, 1, P(mw), P(vw), P(gr), P(st), P(ws),
                                             INF, P(cs), *LR_ARGS, 0, None, ent_coef, 1e-3, 1.0, P(vs), _st()), what)
    gd.check(what)
    return st.cpu(), cs.cpu(), vs.cpu()


@pytest.mark.parametrize("regime", ["A", "B"])
@pytest.mark.parametrize("kind,D,f16,n", SHAPES, ids=wide_ids)
def test_dlogvar_by_probes_against_float64(kind, D, f16, n, regime):
    seed = n % 1000 + D
    actor, critic, flat = _nets(kind, D, seed)
    actor, critic = actor.cpu(), critic.cpu()
    b = probe_batch(actor, critic, kind, D, f16, n, regime, seed)
    g64, g32, bound = probe_reference(actor, b, n)
    what = f"dlogvar probes {kind}-d{D}-{'f16' if f16 else 'f32'}-n{n} regime {regime}"
    st, cs, vs = _var_call(kind, D, f16, n, flat, b, b["adv"], 0.0, what)
    dev, state = float(st[3]), vs.tolist()
    e_dev, e_t32 = dev - g64, g32 - g64
    _pooled.setdefault(regime, []).append((e_dev / bound, e_t32 / bound))
    print(f"{what}: {b['pos'].numel()} probes ({int(b['carrying'].sum())} carrying), float64 {g64:.9e}, device {dev:.9e}; bound {bound:.3e}, "
          f"error / bound: device {abs(e_dev) / bound:.3e}, torch float32 {abs(e_t32) / bound:.3e}; device / float32 "
          f"{abs(e_dev) / abs(e_t32) if e_t32 else math.inf:.3f}")
    assert abs(e_t32) <= 0.1 * bound, "the precondition (tests/test_twins_wide_cpu.py): float32 autograd within a tenth of the bound"
    assert cs[2:].tolist() == [1.0, 1.0]
    assert abs(dev - g64) <= bound, (what, dev, g64, bound)
    assert state[GRAD] == dev and abs(state[GRAD] - g64) <= bound, (what, state[GRAD], dev)   # (coefficient 1, ent_coef 0)
    assert state[STEPS] == 1.0 and state[SKIPPED] == 0.0
    # var_step_kernel's Adam step is the host mirror's on this sum, however many trips it took to add
    ref = ppo.learned_var_reference(ppo.var_state_init(FULL_MANTISSA), dev, float(cs[2]), 0.0, HYPER[0], HYPER[1:3], HYPER[3], 1, 1e-3, 1.0)
    assert [state[i] for i in (THETA, ADAM_M, ADAM_V, GRAD)] == [ref[i] for i in (THETA, ADAM_M, ADAM_V, GRAD)], (what, state, ref)
    if regime == "A":   # adv all zero at the same shape: the sum is exactly 0, the gradient the entropy bonus alone
        st, cs, vs = _var_call(kind, D, f16, n, flat, b, torch.zeros(n), 0.01, what + " adv = 0")
        assert float(vs[GRAD]) == -F32(0.01) and float(st[3]) == 0.0 and float(vs[STEPS]) == 1.0, (what, vs, st)


def test_pooled_error_ratio_is_printed():
    """the device's pooled error over the cases above against PyTorch float32 autograd's (root sums of squares, each error in units of its
    case's bound): printed for profiles/twins_wide.txt, not asserted -- the accuracy gate is test_gpu_learned_var.py's"""
    for regime, rows in sorted(_pooled.items()):
        pd, pt = math.sqrt(sum(d * d for d, _ in rows)), math.sqrt(sum(t * t for _, t in rows))
        print(f"dlogvar probes regime {regime}: {len(rows)} cases, pooled error / bound: device {pd:.3e}, torch float32 {pt:.3e}, "
              f"ratio {pd / pt if pt else math.inf:.3f}")
