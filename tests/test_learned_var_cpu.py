"""PPOConfig.learn_var without a GPU: the host mirror of the device's step of log var against torch.optim.Adam on a float64 scalar, the
PyTorch update path (autograd on log var, the mirror's step), every refusal of the config, the flags of main.py, the checkpoint's
sidecar, the header against the bindings and the C boundary of the three navppo_*_update_epoch_var entry points."""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd.explore_var import ADAM_M, ADAM_V, ENTROPY, GRAD, SKIPPED, STEPS, THETA, VAR
from test_target_kl_cpu import CPU, _batch, _header_decl, _nets

f32 = np.float32
U = 2.0 ** -24
NAN, INF = float("nan"), float("inf")
LOG_2PI = math.log(2.0 * math.pi)
VAR_ENTRIES = ("navppo_mlp64_update_epoch_var", "navppo_mlp64_bf16x3_update_epoch_var", "navppo_resmlp512_update_epoch_var")
BETAS, EPS = (0.9, 0.999), 1e-8


# ------------------------------------------------------------------------------------------------ the mirror
def test_state_init():
    st = ppo.var_state_init(0.8)
    assert len(st) == ppo.VAR_STATE_LEN == 8 and st[VAR] == float(f32(0.8)) and st[THETA] == float(f32(math.log(float(f32(0.8)))))
    assert st[2:] == [0.0] * 6


def test_mirror_against_adam_on_a_float64_scalar():
    """theta stepped by the mirror over 40 steps of varying gradients, coefficients and rates against torch.optim.Adam on a float64
    scalar fed the same float32 gradients: within a few float32 roundings per step of the terms of each update"""
    rng = np.random.default_rng(3)
    theta64 = torch.tensor(math.log(float(f32(0.8))), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([theta64], lr=1e-3, betas=BETAS, eps=EPS)
    state, ent = ppo.var_state_init(0.8), 0.01
    for step in range(1, 41):
        grad_sum, coef, lr = float(f32(rng.normal() * 0.3)), float(f32(rng.uniform(0.2, 1.0))), float(f32(10 ** rng.uniform(-4, -2)))
        new = ppo.learned_var_reference(state, grad_sum, coef, ent, lr, BETAS, EPS, step, 1e-3, 1.0)
        g = float((f32(grad_sum) - f32(ent)) * f32(coef))
        assert new[GRAD] == g and new[STEPS] == step and new[SKIPPED] == 0.0
        opt.param_groups[0]["lr"] = lr
        theta64.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref = float(theta64.detach())
        assert abs(new[THETA] - ref) <= step * 8 * U * (abs(ref) + lr), (step, new[THETA], ref)
        assert new[VAR] == float(f32(math.exp(new[THETA]))) and new[ENTROPY] == float(f32(2.8378770664093453) + f32(new[THETA]))
        assert all(float(f32(x)) == x for x in new)   # float32 values throughout
        state = new
    assert state[THETA] != ppo.var_state_init(0.8)[THETA]


def test_mirror_first_step_skips_and_clamps():
    s0 = ppo.var_state_init(0.5)
    # Adam's first step moves theta by lr against the gradient's sign, whatever its size
    for g, sign in ((0.3, -1.0), (-2.0, 1.0)):
        s1 = ppo.learned_var_reference(s0, g, 1.0, 0.0, 1e-2, BETAS, EPS, 1, 1e-3, 1.0)
        assert s1[THETA] - s0[THETA] == pytest.approx(sign * 1e-2, rel=1e-4)
    # all-zero gradient sum and ent_coef = c: the gradient is exactly -c, the variance rises
    s1 = ppo.learned_var_reference(s0, 0.0, 1.0, 0.01, 1e-2, BETAS, EPS, 1, 1e-3, 1.0)
    assert s1[GRAD] == -float(f32(0.01)) and s1[VAR] > s0[VAR]
    # coefficient 0 (the actor's step was skipped) or a non-finite gradient: only the skip counter moves
    for gs, coef in ((0.3, 0.0), (NAN, 1.0), (INF, 1.0), (0.3, NAN)):
        sk = ppo.learned_var_reference(s0, gs, coef, 0.01, 1e-2, BETAS, EPS, 1, 1e-3, 1.0)
        assert sk[:6] == s0[:6] and sk[SKIPPED] == 1.0 and sk[ENTROPY] == s0[ENTROPY], (gs, coef)
    # the clamps: theta stays at log var_min / log var_max in float32, the moments still move
    lo = ppo.learned_var_reference(s0, 5.0, 1.0, 0.0, 1e-2, BETAS, EPS, 1, 0.5, 1.0)
    hi = ppo.learned_var_reference(s0, -5.0, 1.0, 0.0, 1e-2, BETAS, EPS, 1, 1e-3, 0.5)
    assert lo[:2] == s0[:2] and hi[:2] == s0[:2] and lo[ADAM_M] > 0 > hi[ADAM_M] and lo[STEPS] == hi[STEPS] == 1.0


# ------------------------------------------------------------------------------------------------ configuration and flags
def test_config_defaults_and_every_refusal():
    cfg = ppo.PPOConfig()
    assert (cfg.learn_var, cfg.ent_coef, cfg.var_min, cfg.var_max) == (False, 0.0, 1e-3, 1.0)
    ok = ppo.PPOConfig(learn_var=True, ent_coef=0.01, var_min=0.1, var_max=0.9, init_var=0.9, lr_schedule="adaptive", max_grad_norm=0.5,
                       minibatch_size=64)
    assert ok.learn_var
    bad = [dict(learn_var=1), dict(learn_var="yes"), dict(learn_var=None),
           dict(learn_var=True, ent_coef=-0.01), dict(learn_var=True, ent_coef=NAN), dict(learn_var=True, ent_coef=INF),
           dict(learn_var=True, ent_coef="0.1"), dict(learn_var=True, ent_coef=True),
           dict(learn_var=True, var_min=0.0), dict(learn_var=True, var_min=-1.0), dict(learn_var=True, var_min=NAN),
           dict(learn_var=True, var_max=NAN), dict(learn_var=True, var_max=INF), dict(learn_var=True, var_min=0.5, var_max=0.25),
           dict(var_min=0.0), dict(var_max=NAN),   # the bounds are checked whether or not the option is on
           dict(learn_var=True, init_var=1.5), dict(learn_var=True, init_var=1e-4), dict(learn_var=True, init_var=NAN),
           dict(ent_coef=0.01),                    # a fixed variance has no gradient for the bonus to act on
           dict(learn_var=True, target_kl=0.02), dict(learn_var=True, overlap_allreduce=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ppo.PPOConfig(policy="mlp64x2", **kw)
    with pytest.raises(ValueError, match="without learn_var"):
        ppo.PPOConfig(ent_coef=0.01)
    with pytest.raises(ValueError, match="target_kl"):
        ppo.PPOConfig(learn_var=True, target_kl=0.02)
    with pytest.raises(ValueError, match="overlap_allreduce"):
        ppo.PPOConfig(learn_var=True, overlap_allreduce=True)
    with pytest.raises(ValueError, match="2 ranks"):
        ppo.check_learn_var_config(ppo.PPOConfig(learn_var=True), world=2)
    ppo.check_learn_var_config(ppo.PPOConfig(), world=2)   # off: any number of ranks
    assert ppo.PPOConfig(init_var=1.5).init_var == 1.5     # the clamps bind the learned variance only
    # a config is mutable: the updater checks again
    a, c = _nets()
    cfg = ppo.PPOConfig(policy="mlp64x2", learn_var=True)
    cfg.init_var = 2.0
    with pytest.raises(ValueError, match="outside"):
        ppo.PPOUpdater(a, c, cfg, None, CPU)
    cfg = ppo.PPOConfig(policy="mlp64x2", learn_var=True)
    cfg.target_kl = 0.02
    with pytest.raises(ValueError, match="target_kl"):
        ppo.PPOUpdater(a, c, cfg, None, CPU)


def test_cli_flags_reach_the_config():
    from navbot_ppo_amd import main as cli
    cfg = cli.config_of(cli.get_args([]), 8)
    assert (cfg.learn_var, cfg.ent_coef, cfg.var_min, cfg.var_max) == (False, 0.0, 1e-3, 1.0)
    cfg = cli.config_of(cli.get_args(["--learn_var", "--ent_coef", "0.01", "--var_min", "0.05", "--var_max", "0.9"]), 8)
    assert (cfg.learn_var, cfg.ent_coef, cfg.var_min, cfg.var_max) == (True, 0.01, 0.05, 0.9)
    with pytest.raises(ValueError, match="without learn_var"):
        cli.config_of(cli.get_args(["--ent_coef", "0.01"]), 8)
    with pytest.raises(ValueError, match="target_kl"):
        cli.config_of(cli.get_args(["--learn_var", "--target_kl", "0.02"]), 8)


# ------------------------------------------------------------------------------------------------ the PyTorch formulation
def _updater(n_ep=5, **kw):
    a, c = _nets()
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, learn_var=True, init_var=0.6, **kw), None, CPU)
    calls, lrs = [], []
    step = up._var_step_host

    def recording(grad_sum, coef):
        calls.append((grad_sum, coef))
        lrs.append(up.opt.param_groups[0]["lr"])
        return step(grad_sum, coef)
    up._var_step_host = recording
    return up, _batch(a), calls, lrs


def _theta_grad64(actor, batch, var, adv):
    """d(actor loss)/d(log var) by float64 autograd on `actor` and the advantages `adv`"""
    import copy
    obs, acts, logp, rtg, _ = batch
    a64 = copy.deepcopy(actor).double()
    theta = torch.tensor(math.log(var), dtype=torch.float64, requires_grad=True)
    lp = ppo.gaussian_log_prob(a64(obs.double()), acts.double(), torch.exp(theta))
    ratio = torch.exp(lp - logp.double())
    loss = (-torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv)).mean()
    loss.backward()
    return float(theta.grad)


@pytest.mark.parametrize("max_grad_norm,minibatch_size,lr_schedule", [(None, None, None), (0.5, None, None), (None, 256, None),
                                                                      (0.5, None, "adaptive"), (None, None, "linear")])
def test_pytorch_path_steps_log_var_through_the_mirror(max_grad_norm, minibatch_size, lr_schedule):
    K = 4 if minibatch_size else 1
    up, batch, calls, lrs = _updater(ent_coef=0.01, max_grad_norm=max_grad_norm, minibatch_size=minibatch_size, minibatch_shuffle="none",
                                     lr_schedule=lr_schedule)
    assert up.fused is None and up.mode == "_var" and up.var_state.tolist() == ppo.var_state_init(0.6)
    if lr_schedule == "linear":
        up.set_lr(1e-4)
    a0 = [p.detach().clone() for p in up.actor.parameters()]
    st = up.update(*batch)   # (the `var` of the batch is not read: the state's is)
    assert len(calls) == 5 * K
    # the first step's gradient is autograd's: against float64 on the start policy and the normalised advantages
    if K == 1:
        import copy
        a_start = copy.deepcopy(up.actor)
        with torch.no_grad():
            for p, q in zip(a_start.parameters(), a0):
                p.copy_(q)
        g64 = _theta_grad64(a_start, batch, float(f32(0.6)), up._last_adv.double())
        assert calls[0][0] == pytest.approx(g64, rel=1e-4, abs=1e-6)
    # the state is the mirror replayed over the recorded sums, coefficients and rates
    state = ppo.var_state_init(0.6)
    for k, ((gs, coef), lr) in enumerate(zip(calls, lrs)):
        state = ppo.learned_var_reference(state, gs, coef, 0.01, lr, ppo.ADAM_HYPER[:2], ppo.ADAM_HYPER[2], k + 1, 1e-3, 1.0)
    assert up.var_state.tolist() == state and state[STEPS] == 5 * K
    assert all(c == 1.0 for _, c in calls) if max_grad_norm is None else all(0.0 < c <= 1.0 for _, c in calls)
    if lr_schedule == "adaptive":   # the rate of every step of log var is the one the nets stepped with: the rule replayed over the run's kl
        lr, want = 3e-4, []
        for k, kl in enumerate(up.kl_steps.tolist()):
            lr = ppo.adaptive_lr_reference(lr, kl, 0.01, 1e-5, 1e-2, adapt=k > 0)
            want.append(lr)
        assert lrs == want and st["lr"] == lrs[-1]
    if lr_schedule == "linear":
        assert lrs == [1e-4] * 5
    assert st["var"] == state[VAR] and st["std"] == math.sqrt(state[VAR]) and st["var_grad"] == state[GRAD] and st["var_steps_skipped"] == 0
    assert st["entropy"] == 1.0 + LOG_2PI + state[THETA]
    # a second update goes on from the state and Adam's count
    up.update(*batch)
    assert up.var_state[STEPS] == 10 * K and up._var_t == 10 * K


def test_entropy_bonus_raises_the_variance_and_off_is_the_plain_update():
    up, batch, calls, _ = _updater(ent_coef=50.0)
    up.update(*batch)
    th = up.var_state.tolist()[THETA]
    assert th == pytest.approx(math.log(0.6) + 5 * 3e-4, abs=2e-5)   # Adam under a gradient of one sign: a step of lr per step
    # off: no key, no state, the weights of the update as it was
    a, c = _nets()
    up0 = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=3), None, CPU)
    st0 = up0.update(*_batch(a))
    assert up0.var_state is None and up0.mode == "" and not {"var", "std", "entropy", "var_grad", "var_steps_skipped"} & set(st0)


def test_a_nan_advantage_skips_log_var_with_the_actor():
    up, batch, calls, _ = _updater(n_ep=2, max_grad_norm=0.5)
    obs, acts, logp, rtg, var = batch
    adv = torch.randn(obs.shape[0])
    adv[7] = NAN
    st = up.update(obs, acts, logp, rtg, var, adv_raw=adv, V0=torch.zeros(obs.shape[0]))
    s = up.var_state.tolist()
    assert s[:6] == ppo.var_state_init(0.6)[:6] and s[SKIPPED] == 2.0 and st["var_steps_skipped"] == 2 and st["skipped_steps_actor"] == 2
    assert [c for _, c in calls] == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ log line and scalars
def test_log_line_and_tensorboard_scalars():
    from navbot_ppo_amd import train_log
    lg = dict(iteration=1, t_so_far=10, avg_ep_rews=0.0, success_rate=0.0, avg_ep_lens=0.0, actor_loss=0.0, critic_loss=0.0, approx_kl=0.0,
              steps_per_sec=1.0, rollout_time=0.0, update_time=0.0)
    assert "var_grad" not in train_log.progress_line(lg) and "ppo/var_grad" not in train_log.tb_scalars(lg, ppo.PPOConfig())
    lv = dict(lg, var=0.5, std=math.sqrt(0.5), entropy=1.0 + LOG_2PI + math.log(0.5), var_grad=-0.0123, var_steps_skipped=1)
    line = train_log.progress_line(lv)
    assert " var=0.5000 std=0.7071 entropy=2.1447 var_grad=-1.230e-02 var_steps_skipped=1" in line
    sc = train_log.tb_scalars(lv, ppo.PPOConfig(learn_var=True))
    assert (sc["ppo/var"], sc["ppo/std"], sc["ppo/var_grad"], sc["ppo/var_steps_skipped"]) == (0.5, math.sqrt(0.5), -0.0123, 1)
    assert sc["ppo/entropy"] == pytest.approx(lv["entropy"], abs=1e-12)


# ------------------------------------------------------------------------------------------------ the checkpoint's file
def _bare_trainer(tmp_path, **cfg):
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg = ppo.PPOConfig(output_dir=str(tmp_path), method_name="m", policy="mlp64x2", **cfg)
    t.actor, t.critic = nets.make_policy("mlp64x2")
    t.updater = ppo.PPOUpdater(t.actor, t.critic, t.cfg, None, CPU)
    t.i_so_far, t.t_so_far = 4, 19876
    return t


def test_checkpoint_roundtrip_of_the_variance(tmp_path):
    t = _bare_trainer(tmp_path, learn_var=True, ent_coef=0.01)
    st = ppo.var_state_init(0.8)
    for k in range(3):
        st = ppo.learned_var_reference(st, 0.2 * (k - 1), 0.9, 0.01, 3e-4, BETAS, EPS, k + 1, 1e-3, 1.0)
    t.updater.var_state.copy_(torch.tensor(st))
    view = t.updater.var_state[1]
    pa, pc = t.save_checkpoint()
    d = os.path.dirname(pa)
    assert sorted(os.listdir(d)) == ["actor_iter0004_step00019876.pth", "critic_iter0004_step00019876.pth", "explore_iter0004_step00019876.pth"]
    assert torch.load(os.path.join(d, "explore_iter0004_step00019876.pth")) == {"theta": st[THETA], "m": st[ADAM_M], "v": st[ADAM_V], "steps": 3.0}
    t2 = _bare_trainer(tmp_path, learn_var=True, ent_coef=0.01)
    view2, ptr2 = t2.updater.var_state[1], t2.updater.var_state.data_ptr()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t2.load_checkpoint(pa, pc)
    s2 = t2.updater.var_state.tolist()
    assert [s2[k] for k in (THETA, ADAM_M, ADAM_V, STEPS)] == [st[k] for k in (THETA, ADAM_M, ADAM_V, STEPS)]
    assert s2[VAR] == pytest.approx(st[VAR], rel=1e-6) and s2[SKIPPED] == 0.0 and s2[ENTROPY] == pytest.approx(st[ENTROPY], rel=1e-6)
    assert t2.updater.var_state.data_ptr() == ptr2 and float(view2) == s2[VAR] and float(view) == st[VAR]   # restored in place: views hold


def test_a_missing_variance_file_warns_and_starts_at_init_var(tmp_path):
    off = _bare_trainer(tmp_path)   # the option off: two files, as before
    pa, pc = off.save_checkpoint()
    assert len(os.listdir(os.path.dirname(pa))) == 2
    on = _bare_trainer(tmp_path, learn_var=True, init_var=0.5)
    on.updater.var_state[0] = -3.0
    with pytest.warns(UserWarning, match="explore_iter0004_step00019876.pth not found") as rec:
        on.load_checkpoint(pa, pc)
    assert len(rec) == 1 and "\n" not in str(rec[0].message) and "init_var = 0.5" in str(rec[0].message)
    assert on.updater.var_state.tolist() == ppo.var_state_init(0.5)


# ------------------------------------------------------------------------------------------------ header, bindings, build, C boundary
def test_header_declares_what_the_bindings_bind():
    from navbot_ppo_amd import _native
    bound = {n: args for n, _, args in _native.SYMBOLS}
    ctype_of = lambda a: (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float ") else
                          ctypes.c_int64 if a.startswith("int64_t ") else ctypes.c_int32 if a.startswith("int32_t ") else None)
    for name in VAR_ENTRIES:
        args = _header_decl(name)
        assert name in bound, name
        assert [ctype_of(a) for a in args] == list(bound[name]), (name, args)
        twin = _header_decl(name[:-4] + "_lr")
        # the adaptive-rate twin's arguments without the by-value var, with the four new ones in front of stream
        assert "float var" in twin
        want = [a for a in twin[:-1] if a != "float var"] + ["float ent_coef", "float var_min", "float var_max", "float* var_state_dev"] + twin[-1:]
        assert args == want, (name, args)
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "navppo.h")).read()
    for phrase in ("Learned exploration variance ON THE DEVICE", "var_state_dev [8] f32", "not counted in the actor's norm", "lr_state_dev  may be NULL"):
        assert phrase in txt, phrase
    assert _native.NAVSIM_ABI_VERSION == 6


def test_the_twins_build_with_their_partners_flags():
    from navbot_ppo_amd import build
    assert build.EXTRA_FLAGS["ppo_resmlp512_var.hip"] == build.EXTRA_FLAGS["ppo_resmlp512.hip"]
    assert build.FALLBACK_FLAGS["ppo_resmlp512_var.hip"] == build.FALLBACK_FLAGS["ppo_resmlp512.hip"]
    assert build.per_source_flags("ppo_mlp64_var.hip") == [] and build.per_source_flags("ppo_learned_var.hip") == []
    names = [os.path.basename(s) for s in build.SRCS]
    assert {"ppo_mlp64_var.hip", "ppo_resmlp512_var.hip", "ppo_learned_var.hip"} <= set(names)


def test_library_exports_the_var_entry_points_and_checks_their_arguments():
    from navbot_ppo_amd import _native
    assert os.path.exists(_native.LIB_PATH), "run __graft_entry__.build() first"
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    hyper = (3e-4, 0.9, 0.999, 1e-8)
    good = dict(ent_coef=0.01, var_min=1e-3, var_max=1.0, state=p, max_norm=INF, lr_state=None, kl_target=0.01, adapt=0)
    bad = [dict(state=None), dict(state=ctypes.c_void_p(base + 4)), dict(state=ctypes.c_void_p(base + 8)),
           dict(ent_coef=-1.0), dict(ent_coef=NAN), dict(ent_coef=INF), dict(var_min=0.0), dict(var_min=-1.0), dict(var_min=NAN),
           dict(var_max=1e-4), dict(var_max=NAN), dict(var_max=INF), dict(var_min=INF, var_max=INF)]
    for name, head in (("navppo_mlp64_update_epoch_var", (p, p, 16, 0)), ("navppo_mlp64_bf16x3_update_epoch_var", (p, p, 16)),
                       ("navppo_resmlp512_update_epoch_var", (p, p, 0))):
        assert hasattr(L, name), name
        call = lambda a: getattr(L, name)(*head, p, p, p, p, 32, 0.2, *hyper, 1, p, p, p, p, p, a["max_norm"], p, a["kl_target"], 1e-5, 1e-2,
                                          a["adapt"], a["lr_state"], a["ent_coef"], a["var_min"], a["var_max"], a["state"], None)
        for change in bad:   # refused before any HIP call: no device is needed
            assert call(dict(good, **change)) == -1, (name, change)
            msg = L.navppo_last_error().decode()
            assert msg.startswith(name + ": ") and "var_state_dev" in msg, (name, change, msg)
        # what the clipped and the adaptive-rate twins refuse is still refused
        assert call(dict(good, max_norm=0.0)) == -1 and b"max_norm" in L.navppo_last_error(), name
        assert call(dict(good, lr_state=p, kl_target=0.0)) == -1 and b"kl_target" in L.navppo_last_error(), name
        assert call(dict(good, lr_state=p, adapt=2)) == -1 and b"adapt" in L.navppo_last_error(), name
    assert not any(buf)
