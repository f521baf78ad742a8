"""PPOConfig.target_kl without a GPU: validation, the PyTorch formulation of the early stop (the check before the step, both nets,
then break) against a hand-written loop, the C boundary of the four navppo_*_kl entry points, and the listings of the gated twins of
the hand-placed streams (mlp64_pass_both_x3s_kl, resmlp_bwd2s_kl<0|1>): hazard-free under tools/verify/mfma_hazard_lint.py and with as
many v_mfma instructions as their ungated originals."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from navbot_ppo_amd import nets, ppo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools", "verify"))
CPU = torch.device("cpu")
KL_ENTRIES = ("navppo_mlp64_update_epoch_kl", "navppo_mlp64_bf16x3_update_epoch_kl", "navppo_resmlp512_update_epoch_kl",
              "navppo_adam_step_kl")


def _batch(actor, n=1024, D=16, seed=12):
    """a batch whose logp_old is the start policy's own log-probability of its actions: approx_kl starts at 0 and grows"""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, D), generator=g)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    rtg = torch.randn(n, generator=g) * 3
    var = torch.tensor(0.6)
    with torch.no_grad():
        logp = ppo.gaussian_log_prob(actor(obs), acts, var)
    return obs, acts, logp, rtg, var


def _nets(seed=0):
    torch.manual_seed(seed)
    return nets.make_policy("mlp64x2")


def _hand_loop(n_ep, limit=None, max_norm=None):
    """ppo.py:305-392 written out: both Adam steps per epoch; `limit`: break BEFORE the step of the first epoch whose approx_kl is not
    <= limit.  Returns (flat weights, per-epoch approx_kl of the epochs whose losses were evaluated, steps taken)."""
    a, c = _nets()
    obs, acts, logp_old, rtg, var = _batch(a)
    with torch.no_grad():
        adv = ppo.normalise_advantages(rtg - c(obs).squeeze(-1))
    opts = [torch.optim.Adam(m.parameters(), lr=3e-4) for m in (a, c)]
    kls, steps = [], 0
    for _ in range(n_ep):
        al, cl, r, lp, _ = ppo.ppo_losses(a, c, obs, acts, logp_old, rtg, adv, var, 0.2)
        kl = float(((r.detach() - 1) - (lp.detach() - logp_old)).mean())
        kls.append(kl)
        if limit is not None and not (kl <= limit):
            break
        for o in opts:
            o.zero_grad()
        al.backward()
        cl.backward()
        if max_norm is not None:
            for m in (a, c):
                torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)
        for o in opts:
            o.step()
        steps += 1
    flat = torch.cat([p.detach().reshape(-1) for m in (a, c) for p in m.parameters()])
    return flat, kls, steps


def _trip_epoch(kls):
    """j (1-based) = the smallest k >= 3 with KL_k > 1.5 max(KL_1 .. KL_{k-1}); the limit in the middle of that gap"""
    for k in range(3, len(kls) + 1):
        lo = max(kls[:k - 1])
        if kls[k - 1] > 1.5 * lo:
            return k, 0.5 * (lo + kls[k - 1])
    raise AssertionError(f"no epoch k >= 3 whose approx_kl exceeds 1.5 x the earlier ones: {kls}")


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_pytorch_path_stops_where_a_hand_written_loop_does(max_grad_norm):
    n_ep = 6
    _, kls, _ = _hand_loop(n_ep, max_norm=max_grad_norm)
    j, limit = _trip_epoch(kls)
    assert j < n_ep
    want, kls_b, steps = _hand_loop(n_ep, limit=limit, max_norm=max_grad_norm)
    assert steps == j - 1 and len(kls_b) == j
    a, c = _nets()
    obs, acts, logp_old, rtg, var = _batch(a)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, target_kl=limit / 1.5,
                                            max_grad_norm=max_grad_norm), None, CPU)
    assert up.fused is None and up.kl_limit == pytest.approx(limit)
    st = up.update(obs, acts, logp_old, rtg, var)
    assert st["kl_stop_epoch"] == j - 1 and st["kl_stopped"] == 1
    # same arithmetic per element; the updater steps one flat tensor, the loop one Adam per net
    torch.testing.assert_close(up.fp.flat, want, rtol=1e-6, atol=1e-8)
    h = up.loss_history
    assert h.shape == (n_ep, 2) and bool(torch.isfinite(h[:j]).all()) and bool(torch.isnan(h[j:]).all())
    assert st["approx_kl"] == pytest.approx(sum(kls_b) / j, rel=1e-4, abs=1e-9)     # the mean over the k_pass = j epochs that ran
    if max_grad_norm is None:
        assert "skipped_steps_actor" not in st and "grad_clip_frac_actor" not in st
    else:   # the tripping epoch (coefficient 0, finite norms) is neither a skipped step nor a clipped epoch
        assert st["skipped_steps_actor"] == 0 and st["skipped_steps_critic"] == 0
        cs = up.clip_stats[:j]
        assert torch.equal(cs[j - 1, 2:], torch.zeros(2)) and bool(torch.isfinite(cs[:, :2]).all()) and bool((cs[:j - 1, 2:] > 0).all())
        assert st["grad_clip_frac_critic"] == pytest.approx(float((cs[:j - 1, 3] < 1).float().sum()) / j)
    # a second update from the moved weights: logp_old is stale now, so the first epoch already trips -- nothing moves
    before = up.fp.flat.clone()
    st = up.update(obs, acts, logp_old, rtg, var)
    assert st["kl_stop_epoch"] == 0 and st["kl_stopped"] == 1 and torch.equal(up.fp.flat, before)


def test_a_limit_never_reached_is_the_plain_update():
    a, c = _nets()
    obs, acts, logp_old, rtg, var = _batch(a)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=4, target_kl=1e6), None, CPU)
    st = up.update(obs, acts, logp_old, rtg, var)
    a2, c2 = _nets()
    ref = ppo.PPOUpdater(a2, c2, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=4), None, CPU)
    st_ref = ref.update(obs, acts, logp_old, rtg, var)
    assert torch.equal(up.fp.flat, ref.fp.flat)
    assert st["kl_stop_epoch"] == 4 and st["kl_stopped"] == 0 and "kl_stop_epoch" not in st_ref
    assert set(st) - set(st_ref) == {"kl_stop_epoch", "kl_stopped"}
    for k in st_ref:
        assert st[k] == pytest.approx(st_ref[k], rel=1e-5, abs=1e-9), k


@pytest.mark.parametrize("bad", [0.0, -0.01, float("nan"), -float("inf")])
def test_target_kl_is_validated_on_the_cpu_too(bad):
    a, c = _nets()
    with pytest.raises(ValueError):
        ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", target_kl=bad), None, CPU)


def test_config_default_conflict_and_cli():
    assert ppo.PPOConfig().target_kl is None
    a, c = _nets()
    with pytest.raises(ValueError, match="overlap_allreduce"):
        ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", target_kl=0.02, overlap_allreduce=True), None, CPU)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", target_kl=0.02), None, CPU)
    assert up.kl_limit == pytest.approx(0.03)        # Stable-Baselines3's factor 1.5
    assert ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", overlap_allreduce=True), None, CPU).kl_limit is None
    from navbot_ppo_amd import main
    assert main.get_args([]).target_kl is None
    assert main.get_args(["--target_kl", "0.02"]).target_kl == 0.02


def test_reporting_keys_reach_the_tensorboard_scalars():
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=6, target_kl=0.02)
    t.logger = dict(kl_stop_epoch=3, kl_stopped=1)
    sc = t.tb_scalars()
    assert sc["ppo/kl_stop_epoch"] == 3 and sc["ppo/kl_stopped"] == 1
    t.logger = {}
    sc = t.tb_scalars()
    assert sc["ppo/kl_stop_epoch"] is None and sc["ppo/kl_stopped"] is None     # (None: not written)


def _header_decl(name):
    txt = open(os.path.join(REPO, "include", "navppo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/navppo.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_what_the_bindings_bind():
    from navbot_ppo_amd import _native
    bound = {n: args for n, _, args in _native.SYMBOLS}
    ctype_of = lambda a: (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float ") else
                          ctypes.c_int64 if a.startswith("int64_t ") else ctypes.c_int32 if a.startswith("int32_t ") else None)
    for name in KL_ENTRIES:
        args = _header_decl(name)
        assert name in bound, name
        assert [ctype_of(a) for a in args] == list(bound[name]), (name, args)
        twin = _header_decl(name[:-3] + "_clipped")
        # exactly the clipped twin's arguments, with kl_limit and kl_state_dev (navppo_adam_step_kl: and kl_dev) in front of stream
        extra = ["float kl_limit", "float* kl_state_dev"] + (["const float* kl_dev"] if name == "navppo_adam_step_kl" else [])
        assert args == twin[:-1] + extra + twin[-1:], (name, args)
    txt = open(os.path.join(REPO, "include", "navppo.h")).read()
    for phrase in ("kl_state_dev", "BOTH nets", "a NaN kl trips"):
        assert phrase in txt, phrase


def test_library_exports_the_kl_entry_points_and_checks_their_arguments():
    from navbot_ppo_amd import _native
    assert os.path.exists(_native.LIB_PATH), "run __graft_entry__.build() first"
    L = _native.lib()
    for name in KL_ENTRIES:
        assert hasattr(L, name), name
    # the argument checks run without a device: kl_limit 0 / negative / NaN and a null state are -1 with a message
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hyper = (3e-4, 0.9, 0.999, 1e-8)
    for bad in (0.0, -1.0, float("nan")):
        assert L.navppo_adam_step_kl(p, p, p, p, 8, 4, 1.0, float("inf"), *hyper, 1, p, bad, p, p, None) == -1
        assert b"kl_limit" in L.navppo_last_error()
    assert L.navppo_adam_step_kl(p, p, p, p, 8, 4, 1.0, float("inf"), *hyper, 1, p, 1.0, None, p, None) == -1
    assert b"kl_state_dev" in L.navppo_last_error()
    assert L.navppo_adam_step_kl(p, p, p, p, 8, 4, 1.0, 0.0, *hyper, 1, p, 1.0, p, p, None) == -1 and b"max_norm" in L.navppo_last_error()
    for name, head in (("navppo_mlp64_update_epoch_kl", (p, p, 16, 0)), ("navppo_mlp64_bf16x3_update_epoch_kl", (p, p, 16)),
                       ("navppo_resmlp512_update_epoch_kl", (p, p, 0))):
        call = lambda kl, state: getattr(L, name)(*head, p, p, p, p, 32, 0.6, 0.2, *hyper, 1, p, p, p, p, p, float("inf"), p, kl, state, None)
        for bad in (0.0, -1.0, float("nan")):
            assert call(bad, p) == -1 and b"kl_limit" in L.navppo_last_error(), name
        assert call(float("inf"), None) == -1 and b"kl_state_dev" in L.navppo_last_error(), name


def _listings(tmp_path, sources):
    """{source: listing path}: the product's flags per source, the compiles side by side"""
    from navbot_ppo_amd import build
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    procs = {}
    for src in sources:
        out = tmp_path / (src + ".s")
        extra = build.EXTRA_FLAGS.get(src, [])
        if extra and not build.flags_accepted(extra):
            pytest.skip("hipcc rejects the allocation flag: the library is built without resmlp_bwd2s and its twin (-DRESMLP_BWD2S=0)")
        procs[src] = (out, subprocess.Popen([build.hipcc()] + flags + list(extra) + ["-I", build.INC, "-I", os.path.join(build.HERE, "csrc"), "-S",
                                                                                  "--cuda-device-only", os.path.join(build.HERE, "csrc", src),
                                                                                  "-o", str(out)], stderr=subprocess.DEVNULL))
    for src, (out, p) in procs.items():
        assert p.wait() == 0, src
    return {src: str(out) for src, (out, _) in procs.items()}


def test_gated_twin_of_the_split_bf16_stream_is_hazard_free_with_the_originals_mfma_count(tmp_path):
    from mfma_hazard_lint import lint
    ls = _listings(tmp_path, ["ppo_mlp64.hip", "ppo_mlp64_kl.hip"])
    n0, bad0 = lint(ls["ppo_mlp64.hip"], "mlp64_pass_both_x3sE")
    n1, bad1 = lint(ls["ppo_mlp64_kl.hip"], "mlp64_pass_both_x3s_klE")
    print(f"mlp64_pass_both_x3s: {n0} v_mfma, {len(bad0)} hazards; mlp64_pass_both_x3s_kl: {n1} v_mfma, {len(bad1)} hazards")
    assert n0 >= 400 and not bad0, bad0[:5]
    assert not bad1, bad1[:5]
    assert n1 == n0
    # the twins' translation unit holds the twins only: the ungated kernels keep the listings of THEIR translation unit
    txt = open(ls["ppo_mlp64_kl.hip"]).read()
    assert "mlp64_pass_both_x3sE" not in txt and "reduce_adam_klILb0" in txt and "mlp64_pass_both_klILi16ELb0" in txt


def test_gated_twins_of_the_512_wide_backward_stream_are_hazard_free_with_the_originals_mfma_count(tmp_path):
    from mfma_hazard_lint import lint
    ls = _listings(tmp_path, ["ppo_resmlp512.hip", "ppo_resmlp512_kl.hip"])
    for inst in ("ILb0", "ILb1"):
        n0, bad0 = lint(ls["ppo_resmlp512.hip"], "resmlp_bwd2s" + inst)
        n1, bad1 = lint(ls["ppo_resmlp512_kl.hip"], "resmlp_bwd2s_kl" + inst)
        print(f"resmlp_bwd2s{inst}: {n0} v_mfma, {len(bad0)} hazards; resmlp_bwd2s_kl{inst}: {n1} v_mfma, {len(bad1)} hazards")
        assert n0 >= 450 and not bad0, (inst, bad0[:5])
        assert not bad1, (inst, bad1[:5])
        assert n1 == n0, inst
    txt = open(ls["ppo_resmlp512_kl.hip"]).read()
    for twin in ("resmlp_fwd_klILi16", "resmlp_fwd_klILi32", "resmlp_e2_klILb0", "resmlp_bwd_klILi16", "resmlp_reduce_klILb0"):
        assert twin in txt, twin


def test_the_twins_build_with_their_partners_flags():
    from navbot_ppo_amd import build
    assert build.EXTRA_FLAGS["ppo_resmlp512_kl.hip"] == build.EXTRA_FLAGS["ppo_resmlp512.hip"]
    assert build.FALLBACK_FLAGS["ppo_resmlp512_kl.hip"] == build.FALLBACK_FLAGS["ppo_resmlp512.hip"]
    assert build.per_source_flags("ppo_mlp64_kl.hip") == []
    names = [os.path.basename(s) for s in build.SRCS]
    assert "ppo_mlp64_kl.hip" in names and "ppo_resmlp512_kl.hip" in names
