"""PPOConfig.max_grad_norm on the CPU: validation, the PyTorch formulation of the clipped epoch (per-net clip_grad_norm_ + Adam, the
non-finite skip with the restored Adam state) against a hand-written one, the trainer's gradient guard (warning line and
grad_diagnostics.txt), and the new C entry points in header / library / ctypes table."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPPED = ["navppo_mlp64_update_epoch_clipped", "navppo_mlp64_bf16x3_update_epoch_clipped", "navppo_resmlp512_update_epoch_clipped",
           "navppo_adam_step_clipped"]
CPU = torch.device("cpu")


def _batch(n, seed, d=16):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, d), generator=g)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    logp = -1.2 - 2.3 * torch.rand(n, generator=g)
    rtg = torch.randn(n, generator=g) * 3
    return obs, acts, logp, rtg


def _updater(max_grad_norm, n_ep=3, seed=0, policy="mlp64x2"):
    torch.manual_seed(seed)
    a, c = nets.make_policy(policy)
    cfg = ppo.PPOConfig(policy=policy, n_updates_per_iteration=n_ep, max_grad_norm=max_grad_norm)
    return ppo.PPOUpdater(a, c, cfg, None, CPU)


def test_default_config_has_no_clipping():
    assert ppo.PPOConfig().max_grad_norm is None
    up = _updater(None)
    assert up.max_norm is None
    st = up.update(*_batch(256, 1), torch.tensor(0.8))
    assert up.clip_stats is None
    # the default path reports exactly the figures it reported before: the clip statistics exist with clipping on only
    assert list(st) == ["actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "value_mean", "actor_grad_norm",
                        "critic_grad_norm", "actor_param_delta", "critic_param_delta"]
    on = _updater(1.0).update(*_batch(256, 1), torch.tensor(0.8))
    assert list(on)[:10] == list(st) and list(on)[10:] == ["grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor",
                                                           "skipped_steps_critic"]
    assert isinstance(on["skipped_steps_actor"], int) and on["skipped_steps_actor"] == 0


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_max_grad_norm_is_validated_on_the_cpu_too(bad):
    a, c = nets.make_policy("mlp64x2")
    with pytest.raises(ValueError):
        ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", max_grad_norm=bad), None, CPU)
    assert _updater(float("inf")).max_norm == float("inf")


def test_infinite_bound_is_the_unclipped_update():
    b = _batch(512, 2)
    u0, u1 = _updater(None), _updater(float("inf"))
    s0, s1 = u0.update(*b, torch.tensor(0.8)), u1.update(*b, torch.tensor(0.8))
    assert torch.equal(u0.fp.flat, u1.fp.flat)
    assert torch.equal(u1.clip_stats[:, 2:], torch.ones(3, 2))
    assert s1["actor_grad_norm"] == pytest.approx(s0["actor_grad_norm"], rel=1e-5)
    assert s1["critic_grad_norm"] == pytest.approx(s0["critic_grad_norm"], rel=1e-5)
    assert s1["grad_clip_frac_actor"] == 0.0 and s1["skipped_steps_critic"] == 0


def _by_hand(batch, var, max_norm, n_ep, seed=0, policy="mlp64x2"):
    """Two nets, two torch.optim.Adam, clip_grad_norm_ per net in every epoch (the reference's order of calls, ppo.py:348-392, with a
    finite bound) from the initial weights _updater(seed=seed) has."""
    torch.manual_seed(seed)
    a, c = nets.make_policy(policy)
    a_params, c_params = list(a.parameters()), list(c.parameters())
    oa, oc = torch.optim.Adam(a_params, lr=3e-4), torch.optim.Adam(c_params, lr=3e-4)
    obs, acts, logp, rtg = batch
    with torch.no_grad():
        adv = ppo.normalise_advantages(rtg - c(obs).squeeze(-1))
    rows = []
    for ep in range(n_ep):
        al, cl, _, _, _ = ppo.ppo_losses(a, c, obs, acts, logp, rtg, adv, var, 0.2)
        row = []
        for k, (loss, params, opt) in enumerate(((al, a_params, oa), (cl, c_params, oc))):
            opt.zero_grad()
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
            if bool(torch.isfinite(norm)):
                opt.step()
            row.append((float(norm), min(1.0, max_norm / (float(norm) + 1e-6)) if math.isfinite(float(norm)) else 0.0))
        rows.append(row)
    flat = torch.cat([p.detach().reshape(-1) for p in a_params + c_params])
    return flat, rows, (oa, oc)


def test_pytorch_path_is_clip_grad_norm_and_adam_per_net():
    n_ep, batch, var = 3, _batch(700, 3), torch.tensor(0.8)
    probe = _updater(float("inf"), n_ep=1)
    probe.update(*batch, var)
    norms = probe.clip_stats[0, :2].sqrt()
    max_norm = 0.5 * float(norms.min())          # both nets clip in every epoch
    up = _updater(max_norm, n_ep)
    want, rows, _ = _by_hand(batch, var, max_norm, n_ep)
    st = up.update(*batch, var)
    np.testing.assert_allclose(up.fp.flat.detach().numpy(), want.numpy(), rtol=0, atol=2e-7)
    for ep in range(n_ep):
        for k in range(2):
            assert float(up.clip_stats[ep, k].sqrt()) == pytest.approx(rows[ep][k][0], rel=1e-5)
            assert float(up.clip_stats[ep, 2 + k]) == pytest.approx(rows[ep][k][1], rel=1e-5)
            assert float(up.clip_stats[ep, 2 + k]) < 1.0
    assert st["grad_clip_frac_actor"] == 1.0 and st["grad_clip_frac_critic"] == 1.0
    assert st["actor_grad_norm"] == pytest.approx(np.mean([r[0][0] for r in rows]), rel=1e-5)
    assert st["critic_grad_norm"] == pytest.approx(np.mean([r[1][0] for r in rows]), rel=1e-5)
    # the clip is visible in Adam's first moment (m = 0.1 g' after one step), not in the parameters: Adam is scale-invariant
    one, ref = _updater(max_norm, 1), _updater(None, 1)
    one.update(*batch, var)
    ref.update(*batch, var)
    m1, m0 = one.opt.state[one.fp.proxy]["exp_avg"], ref.opt.state[ref.fp.proxy]["exp_avg"]
    n_a = one.fp.module_numel[0]
    for k, sl in enumerate((slice(0, n_a), slice(n_a, None))):
        big = m0[sl].abs() > 1e-3 * m0[sl].abs().max()
        np.testing.assert_allclose((m1[sl][big] / m0[sl][big]).numpy(), float(one.clip_stats[0, 2 + k]), rtol=1e-5)


def test_pytorch_path_skips_a_net_with_a_non_finite_gradient_and_restores_adam_state():
    batch, var = _batch(300, 4), torch.tensor(0.8)
    obs, acts, logp, rtg = batch
    up = _updater(1.0, n_ep=2)
    up.update(*batch, var)                        # Adam state exists now
    st0 = {k: v.clone() for k, v in up.opt.state[up.fp.proxy].items() if k != "step"}
    flat0 = up.fp.flat.clone()
    rtg_bad = rtg.clone()
    rtg_bad[7] = float("nan")
    # the advantages are the caller's here, so only the critic's loss sees the NaN
    with torch.no_grad():
        adv_raw = rtg - up.value(obs)
    clean = _updater(1.0, n_ep=2)
    clean.update(*batch, var)
    stats_clean = clean.update(obs, acts, logp, rtg, var, adv_raw=adv_raw)
    stats = up.update(obs, acts, logp, rtg_bad, var, adv_raw=adv_raw)
    n_a = up.fp.module_numel[0]
    assert stats["skipped_steps_critic"] == 2 and stats["skipped_steps_actor"] == 0
    assert torch.equal(up.clip_stats[:, 3], torch.zeros(2)) and not bool(torch.isfinite(up.clip_stats[:, 1]).any())
    assert torch.equal(up.fp.flat[n_a:], flat0[n_a:])
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(up.opt.state[up.fp.proxy][k][n_a:], st0[k][n_a:])
        assert torch.equal(up.opt.state[up.fp.proxy][k][:n_a], clean.opt.state[clean.fp.proxy][k][:n_a])
    assert torch.equal(up.fp.flat[:n_a], clean.fp.flat[:n_a]) and not torch.equal(up.fp.flat[:n_a], flat0[:n_a])
    assert bool(torch.isfinite(up.fp.flat).all())
    assert not math.isfinite(stats["critic_grad_norm"]) and math.isfinite(stats["actor_grad_norm"])
    assert stats_clean["skipped_steps_critic"] == 0
    # a NaN observation row: both nets skip, nothing moves -- also on the very first update (no Adam state to restore yet)
    fresh = _updater(1.0, n_ep=2)
    f0 = fresh.fp.flat.clone()
    obs_bad = obs.clone()
    obs_bad[5, 3] = float("nan")
    s = fresh.update(obs_bad, acts, logp, rtg, var)
    assert s["skipped_steps_actor"] == 2 and s["skipped_steps_critic"] == 2 and torch.equal(fresh.fp.flat, f0)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(fresh.opt.state[fresh.fp.proxy][k], torch.zeros_like(f0))


def _guard_trainer(tmp_path, max_grad_norm):
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=2, max_grad_norm=max_grad_norm, output_dir=str(tmp_path) if tmp_path else "")
    t.ctx, t.i_so_far = ppo.SingleProcessCtx(), 7
    t.updater = _updater(max_grad_norm, n_ep=2)
    return t


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
def test_guard_warns_and_writes_diagnostics_on_the_cpu_path(tmp_path, capsys, max_grad_norm):
    t = _guard_trainer(tmp_path, max_grad_norm)
    obs, acts, logp, rtg = _batch(200, 5)
    good = t.updater.update(obs, acts, logp, rtg, torch.tensor(0.8))
    assert t._grad_guard(good) == [] and capsys.readouterr().out == ""
    assert not os.path.exists(os.path.join(str(tmp_path), "grad_diagnostics.txt"))
    before = t.updater.fp.flat.clone()
    obs_bad = obs.clone()
    obs_bad[0, 0] = float("nan")
    bad = t.updater.update(obs_bad, acts, logp, rtg, torch.tensor(0.8))
    assert t._grad_guard(bad) == ["actor", "critic"]
    out = capsys.readouterr().out
    assert "[WARNING] Actor grad norm invalid: nan at iteration 7. Check grad_diagnostics.txt" in out
    assert "[WARNING] Critic grad norm invalid: nan at iteration 7. Check grad_diagnostics.txt" in out
    txt = open(os.path.join(str(tmp_path), "grad_diagnostics.txt")).read()
    for field in ("[ACTOR GRAD ISSUE] Iteration 7", "[CRITIC GRAD ISSUE] Iteration 7", "Net: actor", "Net: critic", "Actor grad norm:",
                  "Critic loss:", "Skipped steps:", "Advantage stats: mean=", "std=", "min=", "max=", "Clip fraction:"):
        assert field in txt, field
    if max_grad_norm is None:     # the default path only reports: the weights are whatever the update made of them
        assert "skipped_steps_actor" not in bad and "Skipped steps: 0 of 2" in txt
    else:
        assert bad["skipped_steps_actor"] == 2 and bad["skipped_steps_critic"] == 2 and "Skipped steps: 2 of 2" in txt
        assert torch.equal(t.updater.fp.flat, before)


def test_guard_never_raises(tmp_path, capsys):
    t = _guard_trainer(None, None)
    blocker = tmp_path / "file"
    blocker.write_text("x")
    t.cfg.output_dir = str(blocker / "below_a_file")    # cannot be created
    st = dict(actor_grad_norm=0.0, critic_grad_norm=1.0, actor_loss=0.1, critic_loss=float("inf"))
    assert t._grad_guard(st) == ["actor", "critic"]
    assert "[WARNING] Actor grad norm invalid: 0.000000 at iteration 7" in capsys.readouterr().out
    t.cfg.output_dir = ""
    assert t._grad_guard(st) == ["actor", "critic"]


def test_clipped_entry_points_in_header_library_and_ctypes_table():
    from navbot_ppo_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "navppo.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(navppo_[a-z0-9_]+)\s*\(", txt))
    bound = {n: a for n, _, a in _native.SYMBOLS}
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in CLIPPED:
        assert name in declared and name in bound and hasattr(lib, name), name
    # the twins' arguments + (float max_norm, float* clip_stats_dev) in front of the stream
    for twin in ("navppo_mlp64_update_epoch", "navppo_mlp64_bf16x3_update_epoch", "navppo_resmlp512_update_epoch"):
        assert bound[twin + "_clipped"] == bound[twin][:-1] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.navsim_version() == 6


def test_clipped_entry_points_check_their_arguments_without_a_device():
    """max_norm of 0, negative or NaN and a null clip_stats_dev: -1 with a message (checked before anything is launched)."""
    from navbot_ppo_amd import _native
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in (0.0, -2.0, float("nan")):
        assert L.navppo_adam_step_clipped(p, p, p, p, 8, 4, 1.0, bad, 3e-4, 0.9, 0.999, 1e-8, 1, p, None) == -1
        assert b"max_norm" in L.navppo_last_error()
        assert L.navppo_mlp64_update_epoch_clipped(p, p, 16, 0, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, bad, p, None) == -1
        assert b"max_norm" in L.navppo_last_error()
        assert L.navppo_mlp64_bf16x3_update_epoch_clipped(p, p, 16, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, bad, p, None) == -1
        assert b"max_norm" in L.navppo_last_error()
        assert L.navppo_resmlp512_update_epoch_clipped(p, p, 0, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, bad, p, None) == -1
        assert b"max_norm" in L.navppo_last_error()
    assert L.navppo_adam_step_clipped(p, p, p, p, 8, 4, 1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8, 1, None, None) == -1
    assert L.navppo_adam_step_clipped(p, p, p, p, 8, 9, 1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8, 1, p, None) == -1   # n_first > n
    assert L.navppo_mlp64_update_epoch_clipped(p, p, 16, 0, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, 1.0, None, None) == -1
    assert b"clip_stats_dev" in L.navppo_last_error()
    assert L.navppo_mlp64_bf16x3_update_epoch_clipped(p, p, 16, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, 1.0, None, None) == -1
    assert L.navppo_resmlp512_update_epoch_clipped(p, p, 0, p, p, p, p, 8, 0.8, 0.2, 3e-4, 0.9, 0.999, 1e-8, 1, p, p, p, p, p, 1.0, None, None) == -1


def test_cli_passes_max_grad_norm():
    from navbot_ppo_amd import main
    assert main.get_args([]).max_grad_norm is None
    assert main.get_args(["--max_grad_norm", "0.5"]).max_grad_norm == 0.5
