"""The action-noise stream of every sampling kernel against tests/_noise.py, draw by draw.

Every action is clamp(mean + sqrt(var) eps) with eps from mlp64::policy_noise (csrc/mlp64_policy.h): Philox4x32-10 keyed by
(seed, global env id, step) + a float32 Box-Muller.  The five call sites -- navppo_mlp64_act, navppo_resmlp512_act, the 16-env
persistent workgroups of navsim_rollout_mlp64 / navsim_rollout_resmlp512 and the 64-env rollout kernel -- each build `step` and
`gid` themselves.  The draws are recovered EXACTLY from a kernel's outputs with a zero actor: every weight and bias 0 gives
z3 = z4 = 0, so mu0 = 1 / (1 + expf(-0)) = 0.5 and mu1 = tanhf(0) = 0 whatever the observations; with var = 2^-8, sd = sqrtf(var) =
2^-4 exactly and nothing clamps (|e| <= 5.77, |e| / 16 <= 0.36).  Then
    a1 = fmaf(sd, e1, 0) = e1 / 16 bit for bit:    e1 = 16 a1 is the kernel's own float32 draw;
    a0 = float32(0.5 + e0 / 16):                   e0 = 16 (a0 - 0.5) within 2^-21 (half an ulp of [0.5, 1) times 16);
    sigmoid head's bias = -200 ("zero leg"): expf(200) = inf, mu0 = 0 exactly, a0 = max(e0 / 16, 0): every positive e0 bit for bit.

Bound on a recovered draw against the float64 reference: 16 x 2^-24 x max(1, rad) (+ 2^-21 on the mu0 = 0.5 leg).  The Philox words,
u1, u2 and the float32 angle are exact in the reference; the kernel adds at most the OpenCL full-profile errors of logf and sqrtf
(3 ulp each, halved through the square root), 4 ulp of sinf / cosf of a value <= 1 and one product rounding: about 8 x 2^-24 x rad,
doubled for margin.  A keying or Philox fault gives errors of order 1.  Observed maxima: profiles/action_noise_exactness.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import _noise

pytestmark = pytest.mark.gpu

VAR = 2.0 ** -8
REL = 16 * 2.0 ** -24       # asserted: |e_gpu - e_ref| <= REL max(1, rad)
HALF = 2.0 ** -21           # + the recovery error of the mu0 = 0.5 leg
LOG_2PI = 1.8378770664093453
MLP64_PA = lambda d: 64 * d + 64 + 64 * 64 + 64 + 64 + 1 + 64 + 1
MLP64_B3 = lambda d: 64 * d + 64 + 64 * 64 + 64 + 64       # layer3.bias: the sigmoid head's bias
RES_PA, RES_BO1 = 50290, 50290 - 1 - 32 - 1                 # out1.bias


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u32(v):
    """A device scalar holding the 32-bit word v (torch has no uint32 arithmetic: the bits go in as int32)."""
    return torch.from_numpy(np.array([v & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)).cuda()


def _actor(family, d, leg):
    """The zero actor ("half": mu = (0.5, 0)) or the zero actor with the sigmoid head's bias at -200 ("zero": mu = (0, 0))."""
    n, b = (MLP64_PA(d), MLP64_B3(d)) if family == "mlp64" else (RES_PA, RES_BO1)
    flat = torch.zeros(n, device="cuda")
    if leg == "zero":
        flat[b] = -200.0
    return flat


def _report(name, worst):
    print(f"action_noise_exactness {name}: max |e_gpu - e_ref| / max(1, rad) = {worst / 2.0 ** -24:.3f} x 2^-24 "
          f"(asserted: {REL / 2.0 ** -24:.0f} x 2^-24)")


def check_draws(act, seed, gids, step, leg, what=""):
    """act [n, 2] float32 (numpy) of the envs `gids` at `step` under `seed` against the reference draws.  Returns the largest
    |e_gpu - e_ref| / max(1, rad) seen (the recovery allowance of the 0.5 leg taken off first)."""
    _, u1, _, e0, e1 = _noise.action_noise(seed, gids, step)
    scale = np.maximum(1.0, _noise.rad_of(u1))
    assert act.dtype == np.float32 and act.shape == (len(e0), 2)
    d1 = np.abs(_noise.recover_exact(act[:, 1]) - e1)
    assert (d1 <= REL * scale).all(), (what, "e1", float((d1 / scale).max()), int(np.argmax(d1 / scale)))
    worst = float((d1 / scale).max())
    if leg == "half":
        d0 = np.abs(_noise.recover_half(act[:, 0]) - e0)
        assert (d0 <= REL * scale + HALF).all(), (what, "e0", float((d0 / scale).max()), int(np.argmax(d0 / scale)))
        worst = max(worst, float((np.maximum(d0 - HALF, 0.0) / scale).max()))
    else:   # a0 = max(e0 / 16, 0): the positive draws bit for bit, 0 for the negative ones, either within the bound of 0
        g0 = _noise.recover_exact(act[:, 0])
        pos, neg = e0 > REL * scale, e0 < -REL * scale
        assert pos.sum() > len(e0) // 8 and neg.sum() > len(e0) // 8   # both branches of the clamp occur
        assert (g0[neg] == 0.0).all() and (g0 >= 0.0).all(), (what, "a0 below its clamp")
        d0 = np.abs(g0 - e0)[~neg]
        assert (d0 <= (REL * scale)[~neg]).all(), (what, "e0", float((d0 / scale[~neg]).max()))
        worst = max(worst, float((d0 / scale[~neg]).max()))
    return worst


def differ(a, b):
    """Two action arrays come from different draws: a1 = e1 / 16 carries 24 significant bits of the draw, so equal entries are
    chance hits (a repeated stream would make every entry equal)."""
    return float((a[..., 1] == b[..., 1]).mean()) < 0.01


def check_logp(act, mean, logp, what=""):
    """The stored log-prob against the float64 formula on the kernel's own action and mean (tolerance of
    test_fused_act_matches_pytorch_policy_step)."""
    a, m = act.astype(np.float64), mean.astype(np.float64)
    want = -0.5 * ((a - m) ** 2).sum(1) / VAR - LOG_2PI - np.log(VAR)
    np.testing.assert_allclose(logp.astype(np.float64), want, rtol=1e-4, atol=2e-5, err_msg=what)


def launch_act(family, d, f16, n, seed, base, step_base, step_offset, leg):
    """One navppo_*_act launch with in-kernel noise.  Returns (act, logp, mean) as numpy."""
    from navbot_ppo_amd._native import lib
    g = torch.Generator().manual_seed(n + d)
    obs = (torch.rand((n, d), generator=g) * 3.5).cuda()   # the observations do not matter: every weight is 0
    if f16:
        obs = obs.half()
    flat = _actor(family, d, leg)
    var = torch.tensor(VAR, device="cuda")
    act = torch.full((n + 1, 2), 7.0, device="cuda")     # one row of padding: the ragged wave must not write past row n - 1
    logp, mean = torch.full((n + 1,), 7.0, device="cuda"), torch.full((n + 1, 2), 7.0, device="cuda")
    sb = None if step_base is None else _u32(step_base)
    if family == "mlp64":
        rc = lib().navppo_mlp64_act(_p(flat), _p(obs), d, int(f16), None, n, _p(var), seed, base, _p(sb), step_offset,
                                    _p(act), _p(logp), _p(mean), _st())
    else:
        rc = lib().navppo_resmlp512_act(_p(flat), _p(obs), int(f16), None, n, _p(var), seed, base, _p(sb), step_offset,
                                        _p(act), _p(logp), _p(mean), _st())
    assert rc == 0, lib().navppo_last_error()
    torch.cuda.synchronize()
    assert (act[n] == 7.0).all() and logp[n] == 7.0 and (mean[n] == 7.0).all()
    return act[:n].cpu().numpy(), logp[:n].cpu().numpy(), mean[:n].cpu().numpy()


def act_case(family, d, f16, n, seed, base, step_base, step_offset, legs=("half", "zero")):
    """Both legs of one key case against the reference.  Returns ({leg: act}, worst error)."""
    step = ((step_base or 0) + step_offset) & 0xFFFFFFFF
    gids = [base + i for i in range(n)]
    worst, acts = 0.0, {}
    for leg in legs:
        act, logp, mean = launch_act(family, d, f16, n, seed, base, step_base, step_offset, leg)
        what = f"{family} D={d} f16={f16} seed={seed:#x} base={base:#x} step={step:#x} leg={leg}"
        want_mean = np.tile(np.array([0.5 if leg == "half" else 0.0, 0.0], dtype=np.float32), (n, 1))
        assert np.array_equal(mean, want_mean), what
        worst = max(worst, check_draws(act, seed, gids, step, leg, what))
        check_logp(act, mean, logp, what)
        acts[leg] = act
    return acts, worst


N_ACT = 53    # three full 16-env waves and a ragged one
FAMILIES = [("mlp64", 16), ("resmlp512", 16)]


@pytest.mark.parametrize("family,d,f16", [("mlp64", 16, 0), ("mlp64", 42, 0), ("mlp64", 16, 1), ("mlp64", 42, 1),
                                          ("resmlp512", 16, 0), ("resmlp512", 16, 1)])
def test_act_draws_match_the_reference_at_every_instantiation(family, d, f16):
    """Every instantiation of the per-step kernels (row width, row type) draws the reference stream: the baseline key with no step
    counter, and a key with a high seed word, a high env id word and a step counter."""
    _, w0 = act_case(family, d, f16, N_ACT, 9, 0, None, 0)
    _, w1 = act_case(family, d, f16, N_ACT, 0x9E3779B97F4A7C15, (1 << 40) + 3, 5, 2)
    _report(f"navppo_{family}_act D={d} f16={f16}", max(w0, w1))


@pytest.mark.parametrize("family,d", FAMILIES)
def test_act_seed_high_word(family, d):
    """(b) a seed whose low word is 0 -- a dropped high word would give the stream of seed 0 -- and (c) a seed and its word-swapped
    twin: both match the reference and differ from each other."""
    acts, _ = act_case(family, d, 0, N_ACT, 0x9E3779B900000000, 0, 5, 2)
    zero, _ = act_case(family, d, 0, N_ACT, 0, 0, 5, 2, legs=("half",))
    assert differ(acts["half"], zero["half"])
    lo, _ = act_case(family, d, 0, N_ACT, 0x00000000DEADBEEF, 0, 5, 2)
    hi, _ = act_case(family, d, 0, N_ACT, 0xDEADBEEF00000000, 0, 5, 2)
    assert differ(lo["half"], hi["half"])


@pytest.mark.parametrize("family,d", FAMILIES)
def test_act_env_id_words(family, d):
    """(d) env_id_base = 2^32 - 20: the carry of env_id_base + i into counter word 1 happens inside the launch (envs 20..52 have word
    1 = 1); (e) env_id_base = 2^40 + 3: a high counter word on every env -- not the stream of env ids 3, 4, .."""
    act_case(family, d, 0, N_ACT, 9, (1 << 32) - 20, 5, 2)
    hi, _ = act_case(family, d, 0, N_ACT, 9, (1 << 40) + 3, 5, 2)
    lo, _ = act_case(family, d, 0, N_ACT, 9, 3, 5, 2, legs=("half",))
    assert differ(hi["half"], lo["half"])


@pytest.mark.parametrize("family,d", FAMILIES)
def test_act_step_counter(family, d):
    """(f) *step_base_dev + step_offset wraps mod 2^32 (0xFFFFFFF0 + 0x20 = 0x10); (g) only the sum matters: (7, 0) and (0, 7) give
    the same bits; and the counter does reach the stream: step 7 is not step 0."""
    act_case(family, d, 0, N_ACT, 9, 0, 0xFFFFFFF0, 0x20)
    a, _ = act_case(family, d, 0, N_ACT, 9, 0, 7, 0)
    b, _ = act_case(family, d, 0, N_ACT, 9, 0, 0, 7)
    for leg in ("half", "zero"):
        assert np.array_equal(a[leg].view(np.int32), b[leg].view(np.int32))
    c, _ = act_case(family, d, 0, N_ACT, 9, 0, None, 0, legs=("half",))
    assert differ(a["half"], c["half"])


# ---------------------------------------------------------------------------------------------- persistent rollouts
def launch_rollout(entry, n, beams, T, act_seed, env_id_base, step_base, leg):
    """One persistent rollout (navsim_rollout_mlp64 / navsim_rollout_mlp64_hist / navsim_rollout_resmlp512) of T steps on stage_1
    with a zero actor (the scan-history entry: the 42-wide one, on the same 16-column buffers).
    Returns (act [T, n, 2], logp [T, n], info) as numpy / dict."""
    from navbot_ppo_amd._native import check, lib
    from navbot_ppo_amd.env import HIST_DIM, VecEnv
    d = beams + 6
    env = VecEnv(n, map="stage_1", n_beams=beams, max_episode_steps=30, seed=3, env_id_base=env_id_base)
    try:
        sim, dev = env.sim, env.device
        if entry == "navsim_rollout_mlp64_hist":
            flat = _actor("mlp64", HIST_DIM, leg)
        else:
            flat = _actor("mlp64" if entry == "navsim_rollout_mlp64" else "resmlp512", d, leg)
        obs = torch.zeros((T + 1, n, d), device=dev)
        act, logp, rew = torch.full((T, n, 2), 7.0, device=dev), torch.zeros((T, n), device=dev), torch.zeros((T, n), device=dev)
        flags = [torch.zeros((T, n), dtype=torch.uint8, device=dev) for _ in range(3)]
        var, sb = torch.tensor(VAR, device=dev), _u32(step_base)
        sim.reset(obs[0])
        check(getattr(lib(), entry)(sim._h, _p(flat), _p(obs), _p(act), _p(logp), _p(rew), *[_p(f) for f in flags], None, None, None,
                                    _p(var), act_seed, _p(sb), T, _st()), entry)
        torch.cuda.synchronize()
        return act.cpu().numpy(), logp.cpu().numpy(), sim.info()
    finally:
        env.close()


ROLLOUT_SEED = 0x9E3779B97F4A7C15 * 5 + 0xAC7 & 0xFFFFFFFFFFFFFFFF    # the trainer's act seed of seed 5: high word in use


@pytest.mark.parametrize("env_id_base,step_base", [(0, 11), ((1 << 32) - 20, 0xFFFFFFFE)])
@pytest.mark.parametrize("entry,n,beams,epb", [("navsim_rollout_mlp64", 37, 10, None), ("navsim_rollout_mlp64", 37, 36, None),
                                               ("navsim_rollout_mlp64", 73, 10, "64"), ("navsim_rollout_resmlp512", 37, 10, None),
                                               ("navsim_rollout_mlp64_hist", 37, 10, None)])
def test_persistent_rollout_draws_match_the_reference(entry, n, beams, epb, env_id_base, step_base, monkeypatch):
    """act_buf[t, i] of a persistent rollout is the reference draw of (act_seed, env_id_base + i, *step_base + t) for every t and i:
    the 16-env workgroups of both families (two full ones and a ragged one) and the forced 64-env shape (one full workgroup and a
    ragged one) -- once with small keys and once with the carry into counter word 1 inside the shard and the step counter wrapping
    mod 2^32 inside the launch (steps 0xFFFFFFFE, 0xFFFFFFFF, 0)."""
    if epb:
        monkeypatch.setenv("NAVSIM_EPB", epb)   # read by NavSim.__init__ (navsim_set_shape, per handle)
    T, worst = 3, 0.0
    gids = [env_id_base + i for i in range(n)]
    for leg in ("half", "zero"):
        act, logp, inf = launch_rollout(entry, n, beams, T, ROLLOUT_SEED, env_id_base, step_base, leg)
        if entry == "navsim_rollout_mlp64":
            assert (inf["rollout_kind"], inf["rollout_epb"]) == ((2, 64) if epb else (1, 16)), inf
        for t in range(T):
            what = f"{entry} n={n} beams={beams} epb={epb} base={env_id_base:#x} step={step_base:#x}+{t} leg={leg}"
            worst = max(worst, check_draws(act[t], ROLLOUT_SEED, gids, (step_base + t) & 0xFFFFFFFF, leg, what))
            mean = np.tile(np.array([0.5 if leg == "half" else 0.0, 0.0], dtype=np.float32), (n, 1))
            check_logp(act[t], mean, logp[t], what)
        assert differ(act[0], act[1]) and differ(act[1], act[2]) and differ(act[0], act[2])
    _report(f"{entry} beams={beams} epb={epb or 16} base={env_id_base:#x}", worst)


# ---------------------------------------------------------------------------------------------- the trainer's three rollout paths
# (one list with the ids pytest gave the three stacked lists, policy-seed-path; scan_history exists on mlp64x2's persistent path only)
TRAINER_CASES = [(po, s, pa) for pa in ("persistent", "graph", "eager") for s in (0, 0xDEADBEEF) for po in ("mlp64x2", "resmlp512")]  \
    + [("mlp64x2", s, "persistent+history") for s in (0, 0xDEADBEEF)]


@pytest.mark.parametrize("policy,seed,path", TRAINER_CASES, ids=[f"{po}-{s}-{pa}" for po, s, pa in TRAINER_CASES])
def test_trainer_rollouts_advance_the_noise_counter(policy, seed, path):
    """PPOTrainer.rollout called three times: after call k the actions are the reference draws of (tr._act_seed, tr._env_id_base + i,
    (k - 1) T + t) -- on the persistent path, on the hipGraph of per-step launches (warm-up, capture and replay must each advance
    the counter exactly once per executed rollout: `_step_base += T` lives inside the captured graph) and on the eager per-step path.
    No iteration repeats another's noise.  "persistent+history": PPOConfig.scan_history, navsim_rollout_mlp64_hist with the 42-wide
    actor."""
    history = path.endswith("+history")
    path = path.split("+")[0]
    from navbot_ppo_amd import ppo
    from navbot_ppo_amd.env import VecEnv
    N, T = 48, 4
    env = VecEnv(N, map="stage_1", max_episode_steps=30, seed=1, env_id_base=0 if seed == 0 else (1 << 32) - 20)
    try:
        cfg = ppo.PPOConfig(rollout_len=T, max_episode_steps=30, n_updates_per_iteration=1, policy=policy, seed=seed, init_var=2 ** -8,
                            persistent_rollout=path == "persistent", use_graph=path == "graph", scan_history=history)
        tr = ppo.PPOTrainer(env, cfg)
        assert tr.updater.fused and tr.uses_persistent_rollout is (path == "persistent")
        assert tr.scan_history is history and (not history or tr.updater.fp.module_numel[0] == MLP64_PA(42) == 7042)
        assert tr._act_seed == (seed * 0x9E3779B97F4A7C15 + 0xAC7) & 0xFFFFFFFFFFFFFFFF and tr._env_id_base == env.sim.cfg.env_id_base
        tr.updater.fp.flat[:tr.updater.fp.module_numel[0]].zero_()   # the actor slice of the flat buffer: what the kernels read
        gids = [tr._env_id_base + i for i in range(N)]
        seen, worst = [], 0.0
        for k in range(3):
            tr.rollout()
            torch.cuda.synchronize()
            assert float(tr.var) == VAR
            assert (path == "graph") == (tr._graph is not None)
            act = tr.act_buf.cpu().numpy()
            for t in range(T):
                worst = max(worst, check_draws(act[t], tr._act_seed, gids, k * T + t, "half", f"{policy} {path} seed={seed:#x} call {k} t={t}"))
            mean = np.tile(np.array([0.5, 0.0], dtype=np.float32), (T * N, 1))
            check_logp(act.reshape(T * N, 2), mean, tr.logp_buf.cpu().numpy().reshape(-1))
            seen.append(act)
            assert int(tr._step_base) == (k + 1) * T
        for i in range(3):
            for j in range(i + 1, 3):
                assert differ(seen[i], seen[j])
        _report(f"PPOTrainer.rollout {policy} {path}{'+history' if history else ''} seed={seed:#x}", worst)
    finally:
        env.close()
