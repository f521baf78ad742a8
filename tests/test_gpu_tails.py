"""Batch tails, buffer guards, per-sample probes and Adam against float64, for the batched entry points of libnavsim.

The other GPU tests hand every kernel exact-size, 256-byte aligned tensors and compare gradients at a tolerance per tensor that
one sample's share (1/n of a mean) falls below at large n.  Here:
  * guarded calls (tests/_guards.py): every argument inside a larger allocation with poisoned / canary guards, at a 256-byte
    boundary and at exactly the minimum alignment the ABI allows for it; guards bit-identical afterwards, no canary left in what
    the contract says is written, outputs bit-identical between the two placements;
  * probes: batches in which only a few chosen samples carry gradient (adv = 0 and a critic target equal to the value elsewhere),
    so the whole gradient is theirs and a sample dropped, repeated or misread moves a tensor by O(1 / #probes), not by 1 / n;
  * Adam: the in-kernel optimiser step and navppo_adam_step against torch.optim.Adam's formula in float64, step count carried
    over epochs and update() calls."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from _guards import Guards, canary_of, is_canary, run_both
from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd._native import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BENCH_N = 512 * 4096


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    assert rc == 0, f"{what}: rc {rc}: {lib().navppo_last_error().decode()}"


def _obs_align(D, f16):
    """navppo.h: obs rows 16-byte aligned at 16 columns, 8-byte at 42 float32 columns, 4-byte at 42 float16 columns."""
    return 16 if D == 16 else (4 if f16 else 8)


def _mlp64_flat(D, seed, scale=2.0):
    torch.manual_seed(seed)
    a, c = nets.make_policy("mlp64x2", obs_dim=D)
    with torch.no_grad():
        for p in list(a.parameters()) + list(c.parameters()):
            p.mul_(scale)
    return a.to(DEV), c.to(DEV), torch.cat([p.detach().reshape(-1) for m in (a, c) for p in m.parameters()]).contiguous()


def _resmlp_flat(seed, scale=1.0):
    torch.manual_seed(seed)
    a, c = nets.make_policy("resmlp512")
    with torch.no_grad():
        for p in list(a.parameters()) + list(c.parameters()):
            p.mul_(scale)
    a.to(DEV), c.to(DEV)
    fp = [p for m in (a, c) for k, p in m.named_parameters() if ".bn" not in "." + k and not k.startswith("bn")]
    return a, c, torch.cat([p.detach().reshape(-1) for p in fp]).contiguous()


def _rand_batch(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, D), generator=g)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    logp = -1.2 - 2.3 * torch.rand(n, generator=g)
    rtg = torch.randn(n, generator=g) * 3
    adv = torch.randn(n, generator=g)
    return [t.to(DEV) for t in (obs, acts, logp, rtg, adv)]


# ================================================================================================ B: guarded calls, PPO side
MLP64_N = [1, 77, 32 * 8 * 256 + 33, 32 * 4 * 256 * 2 + 5]   # tile tail; grid-stride wrap of 8-wave (D16) / 4-wave (D42, x3s) launches


@pytest.mark.parametrize("D,f16", [(16, 0), (16, 1), (42, 0), (42, 1)])
def test_mlp64_entry_points_guarded(D, f16):
    """navppo_mlp64_{loss_grad, loss_grad_net, update_epoch, value, act} and navppo_mlp64_bf16x3_{prepare, loss_grad, loss_grad_net,
    update_epoch} with every buffer guarded, at 256 bytes and at the header's minimum alignment (obs 16 / 8 / 4 bytes, act and
    noise 8, params 16, the critic slice that ppo.py hands navppo_mlp64_value at +4 PA bytes: 8; float arrays 4)."""
    L = lib()
    a, c, flat = _mlp64_flat(D, 7)
    PA = 64 * D + 4354
    PT = flat.numel()
    ws_bytes = L.navppo_mlp64_workspace_bytes(D)
    oa = _obs_align(D, f16)
    for n in MLP64_N:
        obs, acts, logp, rtg, adv = _rand_batch(n, D, n)
        if f16:
            obs = obs.half()
        prep_bytes = L.navppo_mlp64_bf16x3_prep_bytes(n, D)
        noise = torch.randn((n, 2), device=DEV)
        m0 = torch.rand(PT, device=DEV) * 1e-3
        v0 = torch.rand(PT, device=DEV) * 1e-6
        grad_w = {None: None, 0: torch.arange(PT, device=DEV) < PA, 1: torch.arange(PT, device=DEV) >= PA}
        st_w = {None: torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], dtype=torch.bool), 0: torch.tensor([1, 1, 1, 0, 0, 0, 0, 0], dtype=torch.bool),
                1: torch.tensor([0, 0, 0, 0, 1, 1, 1, 0], dtype=torch.bool)}

        def call(g):
            res = {}
            pr = g.inp(flat, 16)
            o = g.inp(obs, oa)
            ac, lp, rt, ad = g.inp(acts, 8), g.inp(logp, 4), g.inp(rtg, 4), g.inp(adv, 4)
            for x3 in (False, True):
                if x3:
                    prep = g.out((prep_bytes,), torch.uint8, 16, written=torch.zeros(1, dtype=torch.bool))
                    _ok(L.navppo_mlp64_bf16x3_prepare(P(o), D, f16, n, P(prep), _st()), "prepare")
                    oargs, pre = (P(prep), D), "navppo_mlp64_bf16x3_"
                else:
                    oargs, pre = (P(o), D, f16), "navppo_mlp64_"
                for net in (None, 0, 1):   # both nets, then each net's pass ALONE: the other slice and its statistics untouched
                    gr = g.out((PT,), torch.float32, 4, written=grad_w[net], untouched=None if net is None else ~grad_w[net])
                    st = g.out((8,), torch.float32, 4, written=st_w[net], untouched=~st_w[net])
                    ws = g.scratch(ws_bytes, 256)
                    if net is None:
                        _ok(getattr(L, pre + "loss_grad")(P(pr), *oargs, P(ac), P(lp), P(rt), P(ad), n, 0.6, 0.2, P(gr), P(st), P(ws), _st()), pre)
                    else:
                        _ok(getattr(L, pre + "loss_grad_net")(net, P(pr), *oargs, P(ac), P(lp), P(rt), P(ad), n, 0.6, 0.2, P(gr), P(st), P(ws),
                                                              _st()), pre + "_net")
                    res[(x3, net)] = (gr, st)
                for step in (1, 2):
                    pw, mw, vw = g.io(flat, 16), g.io(m0, 4), g.io(v0, 4)
                    gr = g.out((PT,), torch.float32, 4)
                    st = g.out((8,), torch.float32, 4, written=torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], dtype=torch.bool))
                    ws = g.scratch(ws_bytes, 256)
                    _ok(getattr(L, pre + "update_epoch")(P(pw), *oargs, P(ac), P(lp), P(rt), P(ad), n, 0.6, 0.2, 3e-4, 0.9, 0.999, 1e-8,
                                                         step, P(mw), P(vw), P(gr), P(st), P(ws), _st()), pre + "update_epoch")
                    res[(x3, "epoch", step)] = (pw, mw, vw, gr)
            # forward-only critic at +4 PA bytes (the pointer ppo.py passes), and the policy step with explicit / in-kernel noise
            crit = g.inp(flat[PA:], 8)
            val = g.out((n,), torch.float32, 4)
            _ok(L.navppo_mlp64_value(P(crit), P(o), D, f16, n, P(val), _st()), "value")
            res["value"] = val
            var = g.inp(torch.tensor([0.7], device=DEV), 4)
            sb = g.inp(torch.tensor([3], dtype=torch.int32, device=DEV), 4)
            nz = g.inp(noise, 8)
            for k, (nzp, sbp) in enumerate(((nz, None), (None, sb))):
                act = g.out((n, 2), torch.float32, 8)
                lpo = g.out((n,), torch.float32, 4)
                mean = g.out((n, 2), torch.float32, 8)
                _ok(L.navppo_mlp64_act(P(pr), P(o), D, f16, P(nzp), n, P(var), 11, 5, P(sbp), 1, P(act), P(lpo), P(mean), _st()), "act")
                res[("act", k)] = (act, mean)
            return res

        res = run_both(DEV, call, f"mlp64 D={D} f16={f16} n={n}")
        # the one-net passes write exactly the slices of the two-net pass; the epochs' Adam step against float64
        for x3 in (False, True):
            for step in (1, 2):
                pw, mw, vw, gr = res[(x3, "epoch", step)]
                _check_adam(flat, m0, v0, gr.double(), step, pw, mw, vw, 3e-4, what=f"update_epoch x3={x3} step={step}")
            g_both = res[(x3, None)][0]
            assert torch.equal(res[(x3, 0)][0][:PA], g_both[:PA]) and torch.equal(res[(x3, 1)][0][PA:], g_both[PA:])
            assert torch.equal(res[(x3, 0)][1][:3], res[(x3, None)][1][:3]) and torch.equal(res[(x3, 1)][1][4:7], res[(x3, None)][1][4:7])
        with torch.no_grad():
            x = obs.float()
            vr = c(x).squeeze(-1)
            np.testing.assert_allclose(res["value"].cpu().numpy(), vr.cpu().numpy(), rtol=1e-5, atol=1e-5 * (1 + vr.abs().max().item()))
            np.testing.assert_allclose(res[("act", 0)][1].cpu().numpy(), a(x).cpu().numpy(), rtol=1e-5, atol=1e-5)


RES_N = [1, 33, 32 * 8 * 32 + 17, 50001]   # tile tail; 8-wave groups of the widest launch (32 groups) wrapped


@pytest.mark.parametrize("f16", [0, 1])
def test_resmlp512_entry_points_guarded(f16):
    """navppo_resmlp512_{loss_grad, update_epoch, value, act}, guards after every buffer and after workspace_bytes(n); obs / params
    16-byte, act 8-byte, the critic slice at +4 * 50290 bytes (8-byte aligned, as navppo.h allows for value), float arrays 4."""
    L = lib()
    a, c, flat = _resmlp_flat(5)
    PA, PT = 50290, flat.numel()
    for n in RES_N:
        obs, acts, logp, rtg, adv = _rand_batch(n, 16, 100 + n)
        if f16:
            obs = obs.half()
        wsb = L.navppo_resmlp512_workspace_bytes(n)

        def call(g):
            res = {}
            pr, o = g.inp(flat, 16), g.inp(obs, 16)
            ac, lp, rt, ad = g.inp(acts, 8), g.inp(logp, 4), g.inp(rtg, 4), g.inp(adv, 4)
            gr = g.out((PT,), torch.float32, 4)
            st = g.out((8,), torch.float32, 4, written=torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], dtype=torch.bool))
            ws = g.scratch(wsb, 256)
            _ok(L.navppo_resmlp512_loss_grad(P(pr), P(o), f16, P(ac), P(lp), P(rt), P(ad), n, 0.6, 0.2, P(gr), P(st), P(ws), _st()), "loss_grad")
            res["grad"] = gr
            pw, mw, vw = g.io(flat, 16), g.io(torch.zeros_like(flat), 4), g.io(torch.zeros_like(flat), 4)
            gr2 = g.out((PT,), torch.float32, 4)
            st2 = g.out((8,), torch.float32, 4, written=torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], dtype=torch.bool))
            _ok(L.navppo_resmlp512_update_epoch(P(pw), P(o), f16, P(ac), P(lp), P(rt), P(ad), n, 0.6, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1,
                                                P(mw), P(vw), P(gr2), P(st2), P(ws), _st()), "update_epoch")
            crit = g.inp(flat[PA:], 8)
            val = g.out((n,), torch.float32, 4)
            _ok(L.navppo_resmlp512_value(P(crit), P(o), f16, n, P(val), P(ws), _st()), "value")
            res["value"] = val
            var = g.inp(torch.tensor([0.7], device=DEV), 4)
            nz = g.inp(torch.randn((n, 2), generator=torch.Generator(DEV).manual_seed(n), device=DEV), 8)
            for k, nzp in enumerate((nz, None)):
                act = g.out((n, 2), torch.float32, 8)
                lpo = g.out((n,), torch.float32, 4)
                mean = g.out((n, 2), torch.float32, 8)
                _ok(L.navppo_resmlp512_act(P(pr), P(o), f16, P(nzp), n, P(var), 3, 0, None, 0, P(act), P(lpo), P(mean), _st()), "act")
                res[("mean", k)] = mean
            return res

        res = run_both(DEV, call, f"resmlp512 f16={f16} n={n}")
        with torch.no_grad():
            x = obs.float()
            vr = c(x).squeeze(-1)
            np.testing.assert_allclose(res["value"].cpu().numpy(), vr.cpu().numpy(), rtol=2e-5, atol=2e-5 * (1 + vr.abs().max().item()))
            np.testing.assert_allclose(res[("mean", 0)].cpu().numpy(), a(x).cpu().numpy(), rtol=2e-5, atol=1e-5)


def test_episode_sums_guarded():
    """navppo_episode_sums with poisoned flags (0x01 / 0xFF) and INT32_MAX lengths past n, at n that is and is not a multiple of 4
    (the vector path needs n % 4 == 0 and 16-byte aligned int / float buffers: the minimum-alignment placement takes the other)."""
    L = lib()
    for n in (1, 255, 256 * 256 * 4 + 3, 4 * 70001):
        gen = torch.Generator().manual_seed(n)
        ended = (torch.rand(n, generator=gen) < 0.1).to(torch.uint8)
        arrive = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
        done = (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
        eplen = (torch.randint(1, 500, (n,), generator=gen) * ended).to(torch.int32)
        epret = torch.round(torch.randn(n, generator=gen) * 100)   # integers: the float64 sum is exact in any order (the two placements
                                                                   # take the vector and the scalar path at n % 4 == 0)
        e, a_, d = ended.bool(), arrive.bool() & ended.bool(), done.bool() & ended.bool()
        want = torch.tensor([e.sum().item(), a_.sum().item(), (d & ~a_).sum().item(), (e & ~d & ~a_).sum().item(), eplen.sum().item(),
                             (epret.double() * e).sum().item()], dtype=torch.float64)

        def call(g):
            bufs = [g.inp(t.to(DEV), 1) for t in (ended, arrive, done)] + [g.inp(eplen.to(DEV), 4), g.inp(epret.to(DEV), 4)]
            out = g.out((6,), torch.float64, 8)
            ws = g.scratch(256 * 6 * 8, 8)
            _ok(L.navppo_episode_sums(*[P(b) for b in bufs], n, P(out), P(ws), _st()), "episode_sums")
            return out

        out = run_both(DEV, call, f"episode_sums n={n}").cpu()
        assert torch.equal(out[:5], want[:5]), (out, want)
        assert abs(out[5] - want[5]) <= 1e-12 * max(1.0, abs(want[5].item()))


@pytest.mark.parametrize("N", [16 * 37, 1000])   # N % 16 == 0: the T-split scan; otherwise the serial one
def test_return_scans_guarded(N):
    """navsim_rtg_scan / navsim_gae_scan: [T, N] rows with poison past row T - 1, every output guarded; exact=1 bit-identical to the
    serial recurrence, the T-split scan within its one-ulp contract; ret of the GAE scan at lambda = 1 equals the rtg scan."""
    from oracle import navsim_oracle as O
    from test_gpu_parity import assert_rtg_close
    L = lib()
    T = 70
    gen = torch.Generator().manual_seed(N)
    rew = torch.randn((T, N), generator=gen)
    ended = (torch.rand((T, N), generator=gen) < 0.05).to(torch.uint8)
    val = torch.randn((T, N), generator=gen)
    lastv = torch.randn(N, generator=gen)
    ref = O.compute_rtgs_tn(rew.numpy(), ended.numpy(), 0.99)
    for exact in (0, 1):
        def call(g):
            r, e, v, lv = g.inp(rew.to(DEV), 4), g.inp(ended.to(DEV), 1), g.inp(val.to(DEV), 4), g.inp(lastv.to(DEV), 4)
            out = g.out((T, N), torch.float32, 4)
            assert L.navsim_rtg_scan(P(r), P(e), T, N, 0.99, P(out), exact, _st()) == 0
            adv1, ret1 = g.out((T, N), torch.float32, 4), g.out((T, N), torch.float32, 4)
            assert L.navsim_gae_scan(P(r), P(e), P(v), None, T, N, 0.99, 1.0, P(adv1), P(ret1), exact, _st()) == 0
            adv2, ret2 = g.out((T, N), torch.float32, 4), g.out((T, N), torch.float32, 4)
            assert L.navsim_gae_scan(P(r), P(e), P(v), P(lv), T, N, 0.99, 0.95, P(adv2), P(ret2), exact, _st()) == 0
            return out, ret1, adv1

        out, ret1, adv1 = run_both(DEV, call, f"return scans N={N} exact={exact}")
        got = out.cpu().numpy()
        if exact or N % 16:
            np.testing.assert_array_equal(got, ref)
        else:
            assert_rtg_close(got, ref)
        assert torch.equal(ret1, out) and torch.equal(adv1, out - val.to(DEV))


def test_adam_step_guarded_against_float64():
    """navppo_adam_step on buffers of n not a multiple of 256, also at the `lo` offsets of ppo.py's per-net steps (PA floats into the
    flat buffer), with params / m / v guarded and grad poisoned past n; grad_scale 1 and 1/8, zero and tiny gradients (v = 0: eps
    dominates), steps 1, 2, 1000, 10^6 -- against torch.optim.Adam's formula in float64 within a few float32 ulps."""
    L = lib()
    gen = torch.Generator().manual_seed(3)
    for n_total, lo in ((1, 0), (255, 0), (257, 0), (5378 + 5313, 0), (5378 + 5313, 5378), (50290 + 50257, 50290)):
        n = n_total - lo
        p0 = torch.randn(n_total, generator=gen)
        for step, scale, kind in ((1, 1.0, "normal"), (2, 0.125, "normal"), (1000, 1.0, "tiny"), (10 ** 6, 0.125, "zero"), (2, 1.0, "tiny")):
            if kind == "normal":
                g0 = torch.randn(n_total, generator=gen) * 10.0 ** torch.randint(-6, 1, (n_total,), generator=gen).float()
            elif kind == "tiny":
                g0 = torch.randn(n_total, generator=gen) * 1e-20
            else:
                g0 = torch.zeros(n_total)
            fresh = step <= 2 and kind != "normal"
            m0 = torch.zeros(n_total) if fresh else torch.randn(n_total, generator=gen) * 1e-3
            v0 = torch.zeros(n_total) if fresh else torch.rand(n_total, generator=gen) * 1e-6

            def call(g):
                pw, mw, vw = g.io(p0.to(DEV), 4), g.io(m0.to(DEV), 4), g.io(v0.to(DEV), 4)
                gr = g.inp(g0.to(DEV), 4)
                off = lambda t: C.c_void_p(t.data_ptr() + 4 * lo)
                _ok(L.navppo_adam_step(off(pw), off(gr), off(mw), off(vw), n, scale, 3e-4, 0.9, 0.999, 1e-8, step, _st()), "adam_step")
                return pw, mw, vw

            pw, mw, vw = run_both(DEV, call, f"adam_step n={n} lo={lo} step={step}")
            gs = g0.double()[lo:] * float(np.float32(scale))
            _check_adam(p0[lo:], m0[lo:], v0[lo:], gs, step, pw[lo:], mw[lo:], vw[lo:], 3e-4, what=f"adam_step n={n} lo={lo} step={step}")
            assert torch.equal(pw[:lo].cpu(), p0[:lo]) and torch.equal(mw[:lo].cpu(), m0[:lo])


F32 = lambda x: float(np.float32(x))   # the hyperparameters as the C ABI receives them (float)


def _check_adam(p0, m0, v0, g, step, p1, m1, v1, lr, b1=0.9, b2=0.999, eps=1e-8, what=""):
    """torch.optim.Adam (no weight decay, no amsgrad) in float64 from the float32 state (p0, m0, v0) and gradient g, with the float32
    values of lr / betas / eps the kernels receive; the kernel's (p1, m1, v1) within a few float32 ulps of the float64 result (relative
    to the terms of each update, so cancellation is no excuse)."""
    u = 2.0 ** -24
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    p0, m0, v0, g = (t.double().cpu() for t in (p0, m0, v0, g))
    p1, m1, v1 = (t.double().cpu() for t in (p1, m1, v1))
    mr = m0 + (g - m0) * (1 - b1)
    vr = b2 * v0 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = (lr / bc1) * mr / (vr.sqrt() / math.sqrt(bc2) + eps)
    pr = p0 - upd
    tiny = 2.0 ** -124   # (float32 subnormals)
    dm = 4 * u * (b1 * m0.abs() + (1 - b1) * g.abs()) + tiny
    assert bool(((m1 - mr).abs() <= dm).all()), (what, "m", (m1 - mr).abs().max().item())
    assert bool(((v1 - vr).abs() <= 4 * u * vr + tiny).all()), (what, "v", ((v1 - vr).abs() / vr.clamp_min(1e-300)).max().item())
    # the denominator adds eps to sqrt(v) / sqrt(bc2): relative error of upd is a few ulps of the terms
    err = (p1 - pr).abs()
    bound = 2 * u * pr.abs() + 12 * u * upd.abs() + (lr / bc1) * dm / (vr.sqrt() / math.sqrt(bc2) + eps) + tiny
    bad = err > bound
    assert not bool(bad.any()), (what, "params", int(bad.sum()), (err / bound.clamp_min(1e-300)).max().item(), step)


# ================================================================================================ B: guarded calls, simulator side
def _sim(N, B, f16, seed, epb=0, per_env=False, max_steps=7):
    from navbot_ppo_amd import maps
    from navbot_ppo_amd.env import NavSim
    s = NavSim(N, n_beams=B, max_episode_steps=max_steps, auto_reset=True, seed=seed, obs_f16=bool(f16), device=DEV,
               envs_per_workgroup=epb)
    return s


def _map(N, per_env, g):
    from navbot_ppo_amd import maps
    seg = torch.as_tensor(np.asarray(maps.stage_1(), dtype=np.float32))
    if per_env:
        seg = (seg[None] + 0.01 * torch.arange(N, dtype=torch.float32)[:, None, None]).contiguous()
    return g.inp(seg.to(DEV), 16)   # NaN segments (poison) after N * S * 4 floats


def _movers(s, g, M):
    """a tape of M segments per phase (M = 37: padded to 40 rows with NaN segments), P = 7, and per-env phase offsets, both placed by
    the Guards: the tape at 16 bytes (the ABI's minimum), BORROWED where it lies; phase0 at 4 bytes (the library copies it)"""
    from _movers import blade_tape
    P = 7
    tape = g.inp(torch.from_numpy(blade_tape(P, M, pad_to=40 if M == 37 else None, radius=0.45)).to(DEV), 16)
    ph0 = g.inp((torch.arange(s.N, dtype=torch.int32) * 5 % P).to(DEV), 4)
    s.set_movers(tape, ph0)
    assert s._mov_tape.data_ptr() == tape.data_ptr() and s._mov_phase0.data_ptr() == ph0.data_ptr()
    assert (s.movers_period, s.movers_segments) == (P, tape.shape[1])
    inf = s.info()
    assert (inf["step_epb"], inf["step_waves"], inf["seq_epb"], inf["rollout_kind"], inf["rollout_epb"]) == (16, 8, 16, 1, 16), inf


_OLD = [(10, 0, False, 0), (10, 1, True, 0), (36, 0, False, 0), (36, 1, True, 0), (10, 0, False, 8), (10, 0, True, 64), (36, 0, False, 16)]


@pytest.mark.parametrize("B,f16,per_env,epb,mov", [pytest.param(*c, None, id="-".join(str(x) for x in c)) for c in _OLD] +
                         [pytest.param(10, 0, False, 0, 37, id="10-0-False-0-movers37"), pytest.param(10, 1, False, 0, 5, id="10-1-False-0-movers5")])
def test_navsim_step_entry_points_guarded(B, f16, per_env, epb, mov):
    """navsim_reset (masked: unmasked rows keep the canary), navsim_step, navsim_step_seq ([T, N, .] rows, guard after the last row),
    navsim_raycast and navsim_rollout_mlp64 on N that is not a multiple of the picked envs_per_workgroup (read from navsim_get_info,
    other shapes forced with set_shape), per-env maps with NaN segments after N * S * 4.  Buffers at 256 bytes and at the smallest
    alignment the header states (actions 8, obs of the rollout 16) or, where it states none, 16 bytes.  mov: with a mover tape
    (_movers), so the calls launch the *_mov_kernel twins: step_mov, steps_mov, rollout_mov, and the reset / ray cast on the tape."""
    N, T = 1000 + 3, 5
    D = B + 6
    odt = torch.float16 if f16 else torch.float32
    gen = torch.Generator().manual_seed(B + epb)
    acts = torch.stack([torch.rand((T, N), generator=gen), torch.rand((T, N), generator=gen) * 2 - 1], 2).contiguous()
    mask = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8)
    a_, _, flat = _mlp64_flat(D, 1)
    PA = 64 * D + 4354

    def call(g):
        s = _sim(N, B, f16, 5, epb)
        try:
            s.set_map(_map(N, per_env, g))
            if mov:
                _movers(s, g, mov)
            info = s.info()
            assert info["step_epb"] > 0 and N % info["step_epb"] != 0 and N % max(info["rollout_epb"], 1) != 0
            al = 16 if g.minimal else 256
            res = {}
            s.reset(g.out((N, D), odt, al))
            obs_r = g.out((N, D), odt, al, written=mask.bool().to(DEV)[:, None], untouched=~mask.bool().to(DEV)[:, None])
            s.reset(obs_r, g.inp(mask.to(DEV), 1))
            res["reset"] = obs_r
            for t in range(2):
                ac = g.inp(acts[t].to(DEV), 8)
                o, r = g.out((N, D), odt, al), g.out((N,), torch.float32, al)
                d, ar, e = (g.out((N,), torch.uint8, al) for _ in range(3))
                er, el, ep = g.out((N,), torch.float32, al, written=torch.zeros(1, dtype=torch.bool)), \
                    g.out((N,), torch.int32, al, written=torch.zeros(1, dtype=torch.bool)), \
                    g.out((N,), torch.float32, al, written=torch.zeros(1, dtype=torch.bool))
                s.step(ac, o, r, d, ar, e, er, el, ep_path=ep)
                torch.cuda.synchronize()
                for buf in (er, el, ep):   # written exactly where an episode ended
                    cz = is_canary(buf)
                    assert not bool((cz & (e != 0)).any()) and bool(cz[e == 0].all())
                res[("step", t)] = (o, r, d, e)
            tape = g.inp(acts.to(DEV), 8)
            o = g.out((T, N, D), odt, al)
            r = g.out((T, N), torch.float32, al)
            fl = [g.out((T, N), torch.uint8, al) for _ in range(3)]
            s.step_seq(tape, o, r, *fl)
            res["seq"] = (o, r)
            pose = g.inp(torch.stack([torch.linspace(-2, 2, N), torch.linspace(1, -1, N), torch.linspace(0, 6, N)], 1).double().to(DEV), 8)
            rng = g.out((N, B), torch.float32, al)
            assert lib().navsim_raycast(s._h, P(pose), P(rng), _st()) == 0
            res["ray"] = rng
            # the persistent rollout: row 0 of obs_buf in, rows 1..T out; every [T, N, .] output guarded after its last row
            s.reset(res[("step", 1)][0])
            start = torch.cat([res[("step", 1)][0][None], canary_of(odt).to(DEV).expand(T, N, D)]).contiguous()
            ob = g.io(start, 16 if g.minimal else 256)
            pr = g.inp(flat[:PA], 16)
            act = g.out((T, N, 2), torch.float32, 8 if g.minimal else 256)
            lp, rw = g.out((T, N), torch.float32, al), g.out((T, N), torch.float32, al)
            fl = [g.out((T, N), torch.uint8, al) for _ in range(3)]
            var = g.inp(torch.tensor([0.5], device=DEV), 4)
            assert lib().navsim_rollout_mlp64(s._h, P(pr), P(ob), P(act), P(lp), P(rw), *[P(f) for f in fl], None, None, None, P(var), 9,
                                              None, T, _st()) == 0
            torch.cuda.synchronize()
            assert not bool(is_canary(ob[1:]).any())
            res["rollout"] = (ob, act, lp)
            return res
        finally:
            s.close()

    run_both(DEV, call, f"navsim B={B} f16={f16} per_env={per_env} epb={epb} movers={mov}")


def test_navsim_rollout_resmlp512_guarded():
    """navsim_rollout_resmlp512 with [T, N, .] rows guarded after the last row, N not a multiple of its 16 envs per workgroup."""
    _rollout_resmlp512_guarded(None)


@pytest.mark.parametrize("mov", [37, 5])
def test_navsim_rollout_resmlp512_guarded_with_movers(mov):
    """... and rollout_resmlp_mov_kernel: the same call on a handle with a guarded mover tape (_movers)"""
    _rollout_resmlp512_guarded(mov)


def _rollout_resmlp512_guarded(mov):
    N, T = 16 * 9 + 5, 4
    _, _, flat = _resmlp_flat(2)

    def call(g):
        s = _sim(N, 10, 0, 3)
        try:
            s.set_map(_map(N, False, g))
            if mov:
                _movers(s, g, mov)
            o0 = g.out((N, 16), torch.float32, 16 if g.minimal else 256)
            s.reset(o0)
            start = torch.cat([o0[None], canary_of(torch.float32).to(DEV).expand(T, N, 16)]).contiguous()
            ob = g.io(start, 16 if g.minimal else 256)
            pr = g.inp(flat[:50290], 16)
            al = 16 if g.minimal else 256
            act = g.out((T, N, 2), torch.float32, 8 if g.minimal else 256)
            lp, rw = g.out((T, N), torch.float32, al), g.out((T, N), torch.float32, al)
            fl = [g.out((T, N), torch.uint8, al) for _ in range(3)]
            var = g.inp(torch.tensor([0.5], device=DEV), 4)
            assert lib().navsim_rollout_resmlp512(s._h, P(pr), P(ob), P(act), P(lp), P(rw), *[P(f) for f in fl], None, None, None, P(var),
                                                  9, None, T, _st()) == 0
            torch.cuda.synchronize()
            assert not bool(is_canary(ob[1:]).any())
            return ob
        finally:
            s.close()

    run_both(DEV, call, f"rollout_resmlp512 movers={mov}")


# ================================================================================================ C: per-sample probes against float64
def _tile_probes(n, waves, wgs):
    """First and last sample of the tiles at every boundary of a launch of `wgs` persistent workgroups of `waves` waves, each wave
    owning 32-sample tiles in a grid-stride loop (tile stride = wgs * waves): first / second tile, the last wave of workgroup 0 and the
    first of workgroup 1, the last workgroup, the wrap of the tile loop, the last two tiles (the prefetched "next tile")."""
    tiles = (n + 31) // 32
    stride = wgs * waves
    ts = {0, 1, waves - 1, waves, waves + 1, (wgs - 1) * waves, wgs * waves - 1, stride, stride + 1, tiles - 1, tiles - 2, tiles - 3,
          tiles - 1 - stride, ((tiles - 1) // stride) * stride, ((tiles - 1) // stride) * stride + waves - 1}
    out = set()
    for t in ts:
        if 0 <= t < tiles:
            out |= {32 * t, min(32 * t + 31, n - 1)}
    return out


def _probe_positions(n, path, seed):
    """Every position for n <= 129; else the launch-geometry boundaries of the kernels on `path` (constants named below), n - 1 and
    a seeded random sample."""
    if n <= 129:
        return np.arange(n)
    tiles = (n + 31) // 32
    pos = {n - 1}
    if path == "resmlp512":
        # csrc/ppo_resmlp512.hip make_plan: groups = min(ceil(tiles / kWaves=8), kMaxWG / (NSL=4 * 2 nets) = 32), multiple of 8 from 8;
        # fwd / e2 / bwd<16> run 8 waves per workgroup, bwd2s (b2s::SW) 4 waves with its tile-and-a-half prefetch
        g = min((tiles + 7) // 8, 32)
        if g >= 8:
            g &= ~7
        for waves, wgs in ((8, g), (4, 2 * g), (4, g)):
            pos |= _tile_probes(n, waves, wgs)
        pos |= {min(n - 1, 32 * (t + k) + j) for t in (0, tiles - 3) for k in (0, 1, 2) for j in (0, 16, 31)}
    else:
        # csrc/ppo_mlp64.hip plan_pass: workgroups = min(ceil(tiles / kWWaves=8), kWMaxBlocks=256); waves per workgroup: 8 (f32, 16
        # columns: Pad<16>::NW), 4 (f32, 42 columns: MLP64_WIDE_WAVES; x3s::SW of the 16-column split stream = 1024 waves; XPad<42>::NW)
        wgs = min((tiles + 7) // 8, 256)
        for waves in (8, 4):
            pos |= _tile_probes(n, waves, wgs)
    rng = np.random.default_rng(seed)
    pos |= set(rng.integers(0, n, 24).tolist())
    return np.array(sorted(p for p in pos if 0 <= p < n))


def _relu_kinks(net, x, eps):
    W1, b1, W2, b2 = [p.detach().double() for p in list(net.parameters())[:4]]
    z1 = x @ W1.T + b1
    z2 = torch.relu(z1) @ W2.T + b2
    return (z1.abs() < eps).any(1) | (z2.abs() < eps).any(1)


def _leaky_kinks(net, x, eps):
    bad = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    inp = x
    for rb in (net.rb1, net.rb2):
        z1 = rb.fc1(inp)
        z2 = inp + rb.fc2(rb.act(z1))
        bad |= (z1.abs() < eps).any(1) | (z2.abs() < eps).any(1)
        inp = torch.cat([x, rb.act(z2)], 1)
    return bad


def _params64(mod):
    return [p for k, p in mod.named_parameters() if ".bn" not in "." + k and not k.startswith("bn")]


def _draw_rows(a64, c64, k, D, f16, gen, var, kinks, eps=1e-4):
    """k probe candidates away from every kink (float64 view of the rows as stored): obs, act, logp_old (ratio in [0.5, 1.6], not
    within 0.02 of 1 +- clip), adv (0.5 .. 1.5, random sign) and rtg = V - (5 .. 15): every probe pulls the critic the same way, and
    hard enough that the background's float32 residual (summed two million times at the bench batch) stays far below the probes' part."""
    rows = []
    have = 0
    while have < k:
        m = 4 * (k - have) + 8
        x = torch.rand((m, D), generator=gen, dtype=torch.float64)
        x = (x.half() if f16 else x.float()).double().to(DEV)
        act = torch.stack([torch.rand(m, generator=gen), torch.rand(m, generator=gen) * 2 - 1], 1).to(DEV)
        with torch.no_grad():
            lp = ppo.gaussian_log_prob(a64(x), act.double(), var)
            r = 0.5 + 1.1 * torch.rand(m, generator=gen, dtype=torch.float64).to(DEV)
            logp_old = (lp - torch.log(r)).float()
            ratio = torch.exp(lp - logp_old.double())
            V = c64(x).squeeze(-1)
            rtg = (V - 5.0 - 10.0 * torch.rand(m, generator=gen, dtype=torch.float64).to(DEV)).float()
            adv = ((0.5 + torch.rand(m, generator=gen)) * (torch.randint(0, 2, (m,), generator=gen) * 2 - 1)).float().to(DEV)
            ok = ~(kinks(a64, x, eps) | kinks(c64, x, eps)) & ((ratio - 0.8).abs() > 0.02) & ((ratio - 1.2).abs() > 0.02)
        idx = ok.nonzero().squeeze(1)[:k - have]
        rows.append((x[idx], act[idx].float(), logp_old[idx], rtg[idx], adv[idx]))
        have += idx.numel()
    return [torch.cat([r[i] for r in rows]) for i in range(5)]


def _probe_case(path, D, f16, n, seed, var=0.6, clip=0.2):
    """One probe batch through `path` ('f32' | 'bf16x3' on the D-64-64 heads, 'resmlp512'): kernel gradient and statistics against
    float64 autograd.  Background samples (every non-probe position) carry one row x0 with adv = 0 -- their surrogate gradient is
    exactly 0 on both sides -- and rtg0 = float32(V64(x0)), so what they add to the critic's gradient is the float32 residual
    r0 = V32(x0) - rtg0 times ONE direction d = dV64(x0)/dtheta (all background samples are the same row).  The check therefore
    removes the component of the critic's error along d -- asserting its coefficient is within float32 round-off of V,
    |c| <= 2 * 1e-5 * (1 + |V64(x0)|) -- and holds what is left, and the actor's error, to 5e-5 of each tensor's scale.  A probe dropped, counted twice or read
    from the wrong row moves its tensors by ~1 / #probes of their scale (>= 1e-2 here)."""
    L = lib()
    gen = torch.Generator().manual_seed(seed)
    if path == "resmlp512":
        a, c, flat = _resmlp_flat(seed % 7 + 1)
        kinks = _leaky_kinks
    else:
        a, c, flat = _mlp64_flat(D, seed % 7 + 1)
        kinks = _relu_kinks
    a64, c64 = copy.deepcopy(a).double(), copy.deepcopy(c).double()
    var64 = torch.tensor(var, dtype=torch.float64, device=DEV)
    pos = torch.as_tensor(_probe_positions(n, path, seed), device=DEV)
    k = pos.numel()
    px, pa, plo, prt, pad = _draw_rows(a64, c64, k, D, f16, gen, var64, kinks)
    bg = k < n
    if bg:
        x0, a0, lo0, _, _ = _draw_rows(a64, c64, 1, D, f16, gen, var64, kinks)
        with torch.no_grad():
            lp0 = ppo.gaussian_log_prob(a64(x0), a0.double(), var64).float()
            rtg0 = c64(x0).squeeze(-1).float()
    odt = torch.float16 if f16 else torch.float32
    obs = (x0.to(odt).expand(n, D) if bg else torch.empty((n, D), dtype=odt, device=DEV)).contiguous()
    acts = (a0.expand(n, 2) if bg else torch.empty((n, 2), device=DEV)).contiguous()
    logp = (lp0.expand(n) if bg else torch.empty(n, device=DEV)).contiguous()
    rtg = (rtg0.expand(n) if bg else torch.empty(n, device=DEV)).contiguous()
    adv = torch.zeros(n, device=DEV)
    obs[pos], acts[pos], logp[pos], rtg[pos], adv[pos] = px.to(odt), pa, plo, prt, pad
    # every argument guarded, at the minimum alignment navppo.h allows for it
    gd = Guards(DEV, minimal=True)
    host = (flat, obs, logp)
    flat, obs = gd.inp(flat, 16), gd.inp(obs, 16 if path == "resmlp512" else _obs_align(D, f16))
    acts, logp, rtg, adv = gd.inp(acts, 8), gd.inp(logp, 4), gd.inp(rtg, 4), gd.inp(adv, 4)
    grad = gd.out(host[0].shape, torch.float32, 4)
    stats = gd.out((8,), torch.float32, 4, written=torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], dtype=torch.bool))
    scratch = lambda nb: gd.scratch(nb, 256)
    if path == "resmlp512":
        ws = scratch(L.navppo_resmlp512_workspace_bytes(n))
        fn = lambda lg: L.navppo_resmlp512_loss_grad(P(flat), P(obs), int(f16), P(acts), P(lg), P(rtg), P(adv), n, var, clip, P(grad),
                                                     P(stats), P(ws), _st())
    else:
        ws = scratch(L.navppo_mlp64_workspace_bytes(D))
        if path == "bf16x3":
            prep = gd.out((L.navppo_mlp64_bf16x3_prep_bytes(n, D),), torch.uint8, 16, written=torch.zeros(1, dtype=torch.bool))
            _ok(L.navppo_mlp64_bf16x3_prepare(P(obs), D, int(f16), n, P(prep), _st()), "prepare")
            fn = lambda lg: L.navppo_mlp64_bf16x3_loss_grad(P(flat), P(prep), D, P(acts), P(lg), P(rtg), P(adv), n, var, clip, P(grad),
                                                            P(stats), P(ws), _st())
        else:
            fn = lambda lg: L.navppo_mlp64_loss_grad(P(flat), P(obs), D, int(f16), P(acts), P(lg), P(rtg), P(adv), n, var, clip, P(grad),
                                                     P(stats), P(ws), _st())
    _ok(fn(logp), path)
    gd.check(f"{path} D={D} f16={f16} n={n}")
    g = grad.double()
    st = stats.cpu().numpy().astype(np.float64)
    # float64 reference: the probes, plus the background's (tiny) critic term in closed form
    p64 = _params64(a64) + _params64(c64)
    for q in p64:
        q.grad = None
    al, cl, ratios, _, _ = ppo.ppo_losses(a64, c64, px, pa.double(), plo.double(), prt.double(), pad.double(), var64, clip)
    al, cl = al * k / n, cl * k / n
    if bg:
        V0 = c64(x0).squeeze(-1)
        cl = cl + (n - k) / n * ((V0 - rtg0.double()) ** 2).sum()
    (al + cl).backward()
    ref = torch.cat([q.grad.reshape(-1) for q in p64])
    err = g - ref
    PA = sum(q.numel() for q in _params64(a64))
    if bg:
        for q in p64:
            q.grad = None
        c64(x0).sum().backward()
        d = torch.cat([q.grad.reshape(-1) for q in _params64(c64)])
        coef = float((err[PA:] @ d) / (d @ d))
        assert abs(coef) <= 2 * (n - k) / n * 1e-5 * (1 + abs(float(V0.detach()))), (path, n, coef)
        err[PA:] -= coef * d
    off = 0
    net_max = [ref[:PA].abs().max().item(), ref[PA:].abs().max().item()]
    for q in p64:
        m = q.numel()
        # a tensor's scale: its largest entry, floored at 1e-2 of its net's (a single bias whose probe terms nearly cancel is held to
        # the round-off of the terms, not of their sum; a probe missing still moves it by ~1 / #probes of the net's scale)
        scale = max(ref[off:off + m].abs().max().item(), 1e-2 * net_max[0 if off < PA else 1])
        e = err[off:off + m].abs().max().item()
        assert e <= 5e-5 * scale + 1e-12, (path, D, f16, n, tuple(q.shape), e, scale)
        off += m
    assert off == ref.numel()
    assert st[0] == pytest.approx(al.item(), rel=2e-5, abs=1e-9)
    assert st[4] == pytest.approx(cl.item(), rel=2e-5, abs=1e-9)
    k_clip = int(((ratios - 1).abs() > clip).sum())
    assert round(st[2] * n) == k_clip, (path, n, st[2] * n, k_clip)
    if bg:   # clip_frac counts exactly: every other sample clipped (ratio 2 on the background), and all n samples
        lp_alt = host[2].clone()
        lp_alt[0::2] = lp0 - math.log(2.0)
        lp_alt[pos] = plo
        kc = int(((ratios - 1).abs() > clip).sum()) + int(((torch.arange(n, device=DEV) % 2 == 0).sum() - (pos % 2 == 0).sum()))
        _ok(fn(gd.inp(lp_alt, 4)), path)
        gd.check()
        assert round(float(stats[2]) * n) == kc, (path, n, float(stats[2]) * n, kc)
        _ok(fn(gd.inp(host[2] - math.log(4.0), 4)), path)   # every ratio times 4: >= 2
        gd.check()
        assert round(float(stats[2]) * n) == n


RAGGED = [2, 31, 33, 63, 65, 127, 129, 255, 257, 1023, 1025, 4095, 4097, 8191, 8193, 32767, 32769, 50001, 65535, 65537]
BENCH = [BENCH_N - 1, BENCH_N, BENCH_N + 1]


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("D,f16", [(16, 0), (16, 1), (42, 0), (42, 1)])
def test_mlp64_probes_against_float64(arith, D, f16):
    sizes = RAGGED + (BENCH if (D, f16) == (16, 0) else [BENCH_N + 1])
    for n in sizes:
        _probe_case(arith, D, f16, n, seed=n % 1000 + D)


@pytest.mark.parametrize("f16", [0, 1])
def test_resmlp512_probes_against_float64(f16):
    sizes = RAGGED + (BENCH if not f16 else [BENCH_N + 1])
    for n in sizes:
        _probe_case("resmlp512", 16, f16, n, seed=n % 1000 + 3)


# ================================================================================================ D: Adam against float64
@pytest.mark.parametrize("policy,arith", [("mlp64x2", "f32"), ("mlp64x2", "bf16x3"), ("resmlp512", "bf16x3")])
def test_update_epoch_adam_against_float64(policy, arith):
    """The Adam step inside *_update_epoch (reduce_adam<true> / resmlp_reduce<true>) on every fused path: per epoch, the kernel's own
    gradient output applied to the saved params / m / v by torch.optim.Adam's formula in float64 must give the kernel's params, m and
    v within a few float32 ulps -- at steps 1, 2, 3 of the first update() and 4, 5, 6 of the second (the _adam_t carry-over).  And the
    weights after both updates track ONE torch.optim.Adam (float64) that lives across the two calls, fed the kernel's gradients."""
    torch.manual_seed(4)
    a, c = nets.make_policy(policy)
    a.to(DEV), c.to(DEV)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, update_arith=arith, n_updates_per_iteration=3), None, DEV)
    assert up.fused
    n = 3000
    obs, acts, logp, rtg, _ = _rand_batch(n, 16, 8)
    rec = []
    orig = up._fused_epoch

    def spy(*args):
        before = (up.fp.flat.clone(), up._adam_m.clone(), up._adam_v.clone(), up._adam_t + 1)
        orig(*args)
        rec.append(before + (up.fp.flat.clone(), up._adam_m.clone(), up._adam_v.clone(), up.fp.grad.clone()))
    up._fused_epoch = spy
    p64 = torch.nn.Parameter(up.fp.flat.detach().double().clone())
    opt = torch.optim.Adam([p64], lr=F32(up.cfg.lr), betas=(F32(0.9), F32(0.999)), eps=F32(1e-8), foreach=False)
    for _ in range(2):
        up.update(obs, acts, logp, rtg, torch.tensor(0.7, device=DEV))
    assert [r[3] for r in rec] == [1, 2, 3, 4, 5, 6] and up._adam_t == 6
    for p0, m0, v0, step, p1, m1, v1, g in rec:
        _check_adam(p0, m0, v0, g.double(), step, p1, m1, v1, up.cfg.lr, what=f"{policy}/{arith} step {step}")
        p64.grad = g.double()
        opt.step()
    drift = (up.fp.flat.double() - p64.detach()).abs()
    assert bool((drift <= 2.0 ** -24 * 16 * p64.detach().abs() + 1e-8).all()), drift.max().item()   # (a wrong step is ~lr = 3e-4 off)
