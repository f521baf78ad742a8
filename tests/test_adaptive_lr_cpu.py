"""PPOConfig.lr_schedule without a GPU: the host mirror of the device rule over a table of float32 bit patterns, validation, the PyTorch
formulation of "adaptive" (the rate of every optimiser step = the mirror replayed over the run's own approx_kl), "linear" through
learn(), the checkpoint's third file, the header against the bindings and the C boundary of the four navppo_*_lr entry points."""
import ctypes
import os
import types
import warnings

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo
from test_target_kl_cpu import CPU, _batch, _header_decl, _nets

f32 = np.float32
LR_ENTRIES = ("navppo_mlp64_update_epoch_lr", "navppo_mlp64_bf16x3_update_epoch_lr", "navppo_resmlp512_update_epoch_lr",
              "navppo_adam_step_lr")
NAN, INF = float("nan"), float("inf")


def bits(x):
    return int(np.array(x, dtype=np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the mirror
T = 0.01   # desired_kl of the table; float32(2 T) and float32(T / 2) are the thresholds the kernel compares with
T2, TH = float(f32(2.0) * f32(T)), float(f32(0.5) * f32(T))
LR = 3e-4
DOWN, UP = f32(LR) / f32(1.5), f32(LR) * f32(1.5)
TABLE = [  # (lr, kl, lr_min, lr_max, adapt) -> (direction, the float32 result)
    ((LR, 0.03, 1e-5, 1e-2, True), (-1, DOWN)),                               # above 2 x target
    ((LR, float(np.nextafter(f32(T2), f32(1))), 1e-5, 1e-2, True), (-1, DOWN)),   # one ulp above
    ((LR, T2, 1e-5, 1e-2, True), (0, f32(LR))),                               # exactly 2 x target: holds
    ((LR, T, 1e-5, 1e-2, True), (0, f32(LR))),
    ((LR, TH, 1e-5, 1e-2, True), (0, f32(LR))),                               # exactly half the target: holds
    ((LR, float(np.nextafter(f32(TH), f32(0))), 1e-5, 1e-2, True), (1, UP)),  # one ulp below
    ((LR, 1e-4, 1e-5, 1e-2, True), (1, UP)),                                  # below half
    ((LR, 1e-14, 1e-5, 1e-2, True), (1, UP)),                                 # rounding noise is "below half" too: hence adapt=False
    ((LR, 0.0, 1e-5, 1e-2, True), (0, f32(LR))),                              # kl == 0: holds
    ((LR, -0.0, 1e-5, 1e-2, True), (0, f32(LR))),
    ((LR, -1e-7, 1e-5, 1e-2, True), (0, f32(LR))),                            # negative: holds
    ((LR, NAN, 1e-5, 1e-2, True), (-1, DOWN)),                                # NaN: lowers
    ((LR, INF, 1e-5, 1e-2, True), (-1, DOWN)),                                # +inf: lowers
    ((LR, -INF, 1e-5, 1e-2, True), (0, f32(LR))),
    ((LR, 0.03, 2.5e-4, 1e-2, True), (-1, f32(2.5e-4))),                      # the lower clamp is reached ...
    ((2.5e-4, 0.03, 2.5e-4, 1e-2, True), (-1, f32(2.5e-4))),                  # ... and is sticky
    ((LR, 1e-4, 1e-5, 4e-4, True), (1, f32(4e-4))),                           # the upper clamp is reached ...
    ((4e-4, 1e-4, 1e-5, 4e-4, True), (1, f32(4e-4))),                         # ... and is sticky
    ((LR, 0.03, 1e-5, 1e-2, False), (0, f32(LR))),                            # adapt off: nothing moves, whatever the kl
    ((LR, 1e-4, 1e-5, 1e-2, False), (0, f32(LR))),
    ((LR, NAN, 1e-5, 1e-2, False), (0, f32(LR))),
]


@pytest.mark.parametrize("args,want", TABLE)
def test_mirror_table(args, want):
    lr, kl, lo, hi, adapt = args
    got = ppo.adaptive_lr_reference(lr, kl, T, lo, hi, adapt=adapt)
    assert isinstance(got, float) and bits(got) == bits(want[1]) and float(f32(got)) == got, (args, got, want)
    assert ppo.adaptive_lr_direction(kl, T, adapt=adapt) == want[0]


def test_mirror_is_float32_arithmetic():
    """three raises and three lowerings do not return to the start in float32 -- the mirror follows the device, not the reals"""
    lr = LR
    seq = []
    for kl in (1e-4, 1e-4, 1e-4, 0.03, 0.03, 0.03):
        lr = ppo.adaptive_lr_reference(lr, kl, T, 1e-5, 1e-2)
        seq.append(lr)
    x = f32(LR)
    for op in "***///":
        x = x * f32(1.5) if op == "*" else x / f32(1.5)
    assert bits(seq[-1]) == bits(x) and [bits(s) for s in seq[:3]] == [bits(f32(LR) * f32(1.5)), bits(f32(LR) * f32(1.5) * f32(1.5)),
                                                                      bits(f32(LR) * f32(1.5) * f32(1.5) * f32(1.5))]
    assert ppo.adaptive_lr_reference(LR, 1e-4, T, 1e-5, 1e-2, adapt=True) == ppo.adaptive_lr_reference(LR, 1e-4, T, 1e-5, 1e-2)   # default: adapt


# ------------------------------------------------------------------------------------------------ configuration and flags
def test_config_defaults_and_validation():
    cfg = ppo.PPOConfig()
    assert cfg.lr_schedule is None and cfg.desired_kl == 0.01 and cfg.lr_min == 1e-5 and cfg.lr_max == 1e-2
    assert ppo.PPOConfig(lr=0.5).lr == 0.5 and ppo.PPOConfig(lr=0.5, lr_schedule="linear").lr == 0.5   # the clamps bind "adaptive" only
    assert ppo.PPOConfig(lr_schedule="adaptive", lr_min=3e-4, lr_max=3e-4).lr_schedule == "adaptive"
    bad = [dict(lr_schedule="cosine"), dict(lr_schedule=True), dict(lr_schedule="adaptive", target_kl=0.02),
           dict(lr_schedule="adaptive", overlap_allreduce=True), dict(lr_schedule="adaptive", lr=1e-6), dict(lr_schedule="adaptive", lr=0.1),
           dict(lr_schedule="adaptive", lr_min=1e-3, lr_max=1e-4, lr=5e-4)]
    for name in ("desired_kl", "lr_min", "lr_max"):
        bad += [dict(lr_schedule="adaptive", **{name: v}) for v in (0.0, -1.0, NAN)]
    for kw in bad:
        with pytest.raises(ValueError):
            ppo.PPOConfig(policy="mlp64x2", **kw)
    with pytest.raises(ValueError, match="target_kl"):
        ppo.PPOConfig(lr_schedule="adaptive", target_kl=0.02)
    with pytest.raises(ValueError, match="overlap_allreduce"):
        ppo.PPOConfig(lr_schedule="adaptive", overlap_allreduce=True)
    # a config is mutable: the updater checks again
    a, c = _nets()
    cfg = ppo.PPOConfig(policy="mlp64x2", lr_schedule="adaptive")
    cfg.target_kl = 0.02
    with pytest.raises(ValueError, match="target_kl"):
        ppo.PPOUpdater(a, c, cfg, None, CPU)
    cfg = ppo.PPOConfig(policy="mlp64x2", lr_schedule="adaptive")
    cfg.lr = 1.0
    with pytest.raises(ValueError, match="outside"):
        ppo.PPOUpdater(a, c, cfg, None, CPU)


def test_cli_flags_reach_the_config():
    from navbot_ppo_amd import main as cli
    cfg = cli.config_of(cli.get_args([]), 8)
    assert cfg.lr_schedule is None and cfg.desired_kl == 0.01 and cfg.lr_min == 1e-5 and cfg.lr_max == 1e-2
    cfg = cli.config_of(cli.get_args(["--lr_schedule", "adaptive", "--desired_kl", "0.02", "--lr_min", "1e-4", "--lr_max", "1e-3"]), 8)
    assert (cfg.lr_schedule, cfg.desired_kl, cfg.lr_min, cfg.lr_max) == ("adaptive", 0.02, 1e-4, 1e-3)
    assert cli.config_of(cli.get_args(["--lr_schedule", "linear"]), 8).lr_schedule == "linear"
    with pytest.raises(SystemExit):
        cli.get_args(["--lr_schedule", "cosine"])


# ------------------------------------------------------------------------------------------------ the PyTorch formulation
def _updater(n_ep=6, **kw):
    a, c = _nets()
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, **kw), None, CPU)
    used = []
    step = up.opt.step

    def recording_step(*args, **kwargs):
        used.append(up.opt.param_groups[0]["lr"])
        return step(*args, **kwargs)
    up.opt.step = recording_step
    return up, _batch(a), used


def _pilot_target():
    """a desired_kl under which the six steps of an update raise, hold and lower: the pilot's kl grows from 0"""
    up, batch, _ = _updater(lr_schedule="adaptive", lr_min=3e-4, lr_max=3e-4)   # (the rate pinned: a constant-rate run that records its kl)
    up.update(*batch)
    return up.kl_steps.tolist()


@pytest.mark.parametrize("max_grad_norm,minibatch_size", [(None, None), (0.5, None), (None, 256)])
def test_pytorch_path_uses_the_mirrors_rate_at_every_step(max_grad_norm, minibatch_size):
    pilot = _pilot_target()
    assert len(pilot) == 6 and pilot[3] > 0
    K = 4 if minibatch_size else 1
    ok = False
    for mult in (4.0, 2.0, 8.0, 1.0, 16.0, 0.5, 32.0):
        desired = mult * pilot[3]
        up, batch, used = _updater(lr_schedule="adaptive", desired_kl=desired, max_grad_norm=max_grad_norm, minibatch_size=minibatch_size,
                                   minibatch_shuffle="none")
        assert up.fused is None and up.lr_state is None
        st1 = up.update(*batch)
        kls1 = up.kl_steps.tolist()
        dirs = [ppo.adaptive_lr_direction(kl, desired, adapt=k > 0) for k, kl in enumerate(kls1)]
        print(f"desired_kl {mult} x pilot kl[3] = {desired:.3e}: kl {kls1} -> {dirs}")
        if set(dirs) == {-1, 0, 1} or (K > 1 and len(set(dirs)) >= 2):
            ok = True
            break
    assert ok, "no candidate target under which the update both changes and holds the rate"
    assert len(kls1) == 6 * K == len(used)
    lr, want = 3e-4, []
    for k, kl in enumerate(kls1):
        lr = ppo.adaptive_lr_reference(lr, kl, desired, 1e-5, 1e-2, adapt=k > 0)
        want.append(lr)
    assert used == want and used[0] == float(f32(3e-4))            # the first step of the update does not adapt
    assert st1["lr"] == want[-1] and st1["lr_ups"] == sum(d > 0 for d in dirs) and st1["lr_downs"] == sum(d < 0 for d in dirs)
    assert st1["approx_kl"] == pytest.approx(sum(kls1) / len(kls1), rel=1e-5, abs=1e-12)
    # a second update: starts at the first one's final rate, its first step does not adapt (its kl is far from 0 now: stale logp_old)
    del used[:]
    st2 = up.update(*batch)
    kls2 = up.kl_steps.tolist()
    assert used[0] == want[-1] and kls2[0] > 0
    want2 = []
    for k, kl in enumerate(kls2):
        lr = ppo.adaptive_lr_reference(lr, kl, desired, 1e-5, 1e-2, adapt=k > 0)
        want2.append(lr)
    assert used == want2 and st2["lr"] == want2[-1]
    d2 = [ppo.adaptive_lr_direction(kl, desired, adapt=k > 0) for k, kl in enumerate(kls2)]
    assert (st2["lr_ups"], st2["lr_downs"]) == (sum(d > 0 for d in d2), sum(d < 0 for d in d2))   # per update, not cumulative
    if max_grad_norm is None:
        assert "skipped_steps_actor" not in st1
    assert "kl_stop_epoch" not in st1


def test_pinned_rate_and_no_schedule_are_the_plain_update():
    """lr_schedule=None adds no key and moves the weights as before; "adaptive" with lr_min = lr_max = lr steps with that one rate"""
    up0, batch, used0 = _updater(n_ep=4)
    st0 = up0.update(*batch)
    up1, _, used1 = _updater(n_ep=4, lr_schedule="adaptive", lr_min=3e-4, lr_max=3e-4)
    st1 = up1.update(*batch)
    assert used0 == [3e-4] * 4 and used1 == [float(f32(3e-4))] * 4
    assert up0.kl_steps is None and up0.lr_value is None
    assert set(st1) - set(st0) == {"lr", "lr_ups", "lr_downs"} and "lr" not in st0
    torch.testing.assert_close(up1.fp.flat, up0.fp.flat, rtol=1e-6, atol=1e-9)   # (3e-4 against float32(3e-4) in Adam's step size)


def test_linear_schedule_through_learn():
    a, c = _nets()
    cfg = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=2, lr_schedule="linear", rollout_len=8)
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg, t.ctx, t.env = cfg, ppo.SingleProcessCtx(), types.SimpleNamespace(N=8)
    t.updater = ppo.PPOUpdater(a, c, cfg, None, CPU)
    t.t_so_far = t.i_so_far = 0
    t.logger = {}
    batch = _batch(a)
    seen = []

    def iteration():   # (the simulator has no CPU build: an iteration that only updates, 100 completed steps each)
        seen.append((t.t_so_far, t.updater.opt.param_groups[0]["lr"]))
        stats = t.updater.update(*batch)
        t.t_so_far += 100
        t.i_so_far += 1
        t.logger = dict(stats, iteration=t.i_so_far, t_so_far=t.t_so_far, avg_ep_rews=0.0, success_rate=0.0, avg_ep_lens=0.0,
                        steps_per_sec=1.0, rollout_time=0.0, update_time=0.0)
        return t.logger
    t.iteration = iteration
    lines, logs = [], []
    t.learn(500, log=lambda s, **kw: (lines.append(s), logs.append(dict(t.logger))))
    assert len(seen) == 5
    for i, (t_so_far, lr) in enumerate(seen):
        assert t_so_far == 100 * i and lr == 3e-4 * max(0.0, 1.0 - t_so_far / 500) == ppo.linear_lr(3e-4, t_so_far, 500)
        assert logs[i]["lr"] == lr and f" lr={lr:.3e}" in lines[i] and "lr_ups" not in logs[i]
    assert seen[0][1] == 3e-4 and seen[4][1] == pytest.approx(0.6e-4)
    assert ppo.linear_lr(3e-4, 600, 500) == 0.0
    t.logger = logs[-1]
    assert t.tb_scalars()["ppo/lr"] == seen[-1][1] and "ppo/lr_ups" not in t.tb_scalars()
    t.logger = dict(lr=1e-3, lr_ups=2, lr_downs=1)
    sc = t.tb_scalars()
    assert (sc["ppo/lr"], sc["ppo/lr_ups"], sc["ppo/lr_downs"]) == (1e-3, 2, 1)
    t.logger = {}
    assert "ppo/lr" not in t.tb_scalars()


# ------------------------------------------------------------------------------------------------ the checkpoint's file
def _bare_trainer(tmp_path, **cfg):
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg = ppo.PPOConfig(output_dir=str(tmp_path), method_name="m", policy="mlp64x2", **cfg)
    t.actor, t.critic = nets.make_policy("mlp64x2")
    t.updater = ppo.PPOUpdater(t.actor, t.critic, t.cfg, None, CPU)
    t.i_so_far, t.t_so_far = 4, 19876
    return t


def test_checkpoint_roundtrip_of_the_learning_rate(tmp_path):
    t = _bare_trainer(tmp_path, lr_schedule="adaptive")
    assert t.updater.lr_value == 3e-4
    t.updater.set_lr(float(f32(4.5e-4)))
    pa, pc = t.save_checkpoint()
    d = os.path.dirname(pa)
    assert sorted(os.listdir(d)) == ["actor_iter0004_step00019876.pth", "critic_iter0004_step00019876.pth", "lrsched_iter0004_step00019876.pth"]
    assert torch.load(os.path.join(d, "lrsched_iter0004_step00019876.pth")) == {"lr": float(f32(4.5e-4))}
    assert ppo.PPOTrainer.lrsched_path(pa) == os.path.join(d, "lrsched_iter0004_step00019876.pth")
    t2 = _bare_trainer(tmp_path, lr_schedule="adaptive")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t2.load_checkpoint(pa, pc)
    assert t2.updater.lr_value == float(f32(4.5e-4)) == t2.updater.opt.param_groups[0]["lr"]
    for k, v in t.actor.state_dict().items():
        assert torch.equal(v, t2.actor.state_dict()[k])


def test_a_missing_rate_file_warns_and_starts_at_the_configured_rate(tmp_path):
    off = _bare_trainer(tmp_path)   # no schedule: two files, as before
    pa, pc = off.save_checkpoint()
    assert len(os.listdir(os.path.dirname(pa))) == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off.load_checkpoint(pa, pc)
    on = _bare_trainer(tmp_path, lr_schedule="adaptive")
    on.updater.set_lr(1e-3)
    with pytest.warns(UserWarning, match="lrsched_iter0004_step00019876.pth not found") as rec:
        on.load_checkpoint(pa, pc)
    assert len(rec) == 1 and "\n" not in str(rec[0].message)
    assert on.updater.lr_value == 3e-4


# ------------------------------------------------------------------------------------------------ header, bindings, C boundary
def test_header_declares_what_the_bindings_bind():
    from navbot_ppo_amd import _native
    bound = {n: args for n, _, args in _native.SYMBOLS}
    ctype_of = lambda a: (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float ") else
                          ctypes.c_int64 if a.startswith("int64_t ") else ctypes.c_int32 if a.startswith("int32_t ") else None)
    for name in LR_ENTRIES:
        args = _header_decl(name)
        assert name in bound, name
        assert [ctype_of(a) for a in args] == list(bound[name]), (name, args)
        twin = _header_decl(name[:-3] + "_clipped")
        extra = ["float kl_target", "float lr_min", "float lr_max", "int32_t adapt", "float* lr_state_dev"] + (
            ["const float* kl_dev"] if name == "navppo_adam_step_lr" else [])
        assert args == twin[:-1] + extra + twin[-1:], (name, args)
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "navppo.h")).read()
    for phrase in ("Adaptive learning rate ON THE DEVICE", "lr_state_dev  [4] f32", "a NaN kl lowers", "(step + 1) & 1", "Two slots"):
        assert phrase in txt, phrase
    assert _native.NAVSIM_ABI_VERSION == 6


def test_library_exports_the_lr_entry_points_and_checks_their_arguments():
    from navbot_ppo_amd import _native
    assert os.path.exists(_native.LIB_PATH), "run __graft_entry__.build() first"
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hyper = (3e-4, 0.9, 0.999, 1e-8)
    good = dict(kl_target=0.01, lr_min=1e-5, lr_max=1e-2, adapt=1, state=p)
    bad = [dict(kl_target=0.0), dict(kl_target=-1.0), dict(kl_target=NAN), dict(lr_min=0.0), dict(lr_min=-1.0), dict(lr_min=NAN),
           dict(lr_max=1e-6), dict(lr_max=NAN), dict(adapt=2), dict(adapt=-1), dict(state=None)]
    calls = {"navppo_adam_step_lr": lambda a, mn=INF: L.navppo_adam_step_lr(p, p, p, p, 8, 4, 1.0, mn, *hyper, 1, p, a["kl_target"], a["lr_min"],
                                                                            a["lr_max"], a["adapt"], a["state"], p, None)}
    for name, head in (("navppo_mlp64_update_epoch_lr", (p, p, 16, 0)), ("navppo_mlp64_bf16x3_update_epoch_lr", (p, p, 16)),
                       ("navppo_resmlp512_update_epoch_lr", (p, p, 0))):
        calls[name] = lambda a, mn=INF, name=name, head=head: getattr(L, name)(
            *head, p, p, p, p, 32, 0.6, 0.2, *hyper, 1, p, p, p, p, p, mn, p, a["kl_target"], a["lr_min"], a["lr_max"], a["adapt"], a["state"], None)
    for name in LR_ENTRIES:
        assert hasattr(L, name), name
        for change in bad:   # refused before any HIP call: no device is needed
            assert calls[name](dict(good, **change)) == -1, (name, change)
            msg = L.navppo_last_error().decode()
            assert msg.startswith(name + ": ") and "lr_state_dev" in msg, (name, change, msg)
        assert calls[name](good, 0.0) == -1 and b"max_norm" in L.navppo_last_error(), name   # the clipped twin's checks still hold
    assert L.navppo_adam_step_lr(p, p, p, p, 8, 4, 1.0, INF, *hyper, 1, p, 0.01, 1e-5, 1e-2, 1, p, None, None) == -1
    assert b"kl_dev" in L.navppo_last_error()
    assert not any(buf)
