"""The persistent evaluation: navsim_evaluate_mlp64 / navsim_evaluate_resmlp512 (one launch: deterministic HIP actor + env step on
chip, episode quota in LDS, early exit per workgroup), VecEnv.evaluate_policy, evaluate(persistent=True) and PPOConfig.eval_every.

The reference of every table check is written HERE from the per-step entry points: navsim_reset, then per step navppo_mlp64_act /
navppo_resmlp512_act with noise_dev = zeros (policy_finish computes fmaf(sd, 0, mu): exactly the clamped mean) followed by
navsim_step, with the quota rule of evaluate() applied on the host in numpy.  Same device functions on the same inputs, so the
kernel's table must equal it bit for bit -- no tolerance anywhere in this file."""
import csv
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from _guards import run_both
from navbot_ppo_amd import evaluate as ev, maps, nets, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, VecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CAP = 40          # max_episode_steps of the table cases
FILL = 77         # what unreached slots are prefilled with (u8 / i32 / f32)
ENTRY = {"mlp64x2": "navsim_evaluate_mlp64", "resmlp512": "navsim_evaluate_resmlp512"}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _actor(policy, D, seed=5):
    """a random-init actor with spread-out actions (parameters scaled up) and its flat parameters"""
    torch.manual_seed(seed)
    a, _ = nets.make_policy(policy, obs_dim=D)
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(2.0 if policy == "mlp64x2" else 1.5)
    a = a.to(DEV)
    return a, nets.flat_actor_params(a).to(DEV)


def _sim(N, B, f16, map_name, seed, cap=CAP, auto_reset=True, **kw):
    """An evaluation handle (arrival threshold 0.4).  stage_1: the robot starts 0.7 m in front of the inner wall and the goals
    fall in a 1 m box around it, so that arrivals, collisions and time-outs all happen within 40-step episodes; house_base (256
    segments: the tile-box cast): the curated start / goal tables of the house.  kw: further handle options (the sensor's)."""
    if map_name == "stage_1":
        s = NavSim(N, n_beams=B, max_episode_steps=cap, auto_reset=auto_reset, seed=seed, threshold_arrive=0.4, obs_f16=f16,
                   spawn=(1.2, 0.8, 0.0), goal_box=(0.6, 1.6), device=DEV, **kw)
        s.set_map(maps.by_name(map_name))
    else:
        s = NavSim(N, n_beams=B, max_episode_steps=cap, auto_reset=auto_reset, seed=seed, threshold_arrive=0.4, obs_f16=f16, device=DEV,
                   **kw)
        s.set_map(maps.by_name(map_name))
        s.set_spawn_sampler(*maps.spawn_tables("small_house", min_dist=0.3, max_dist=6.0))
    return s


def _act(policy, flat, obs, D, f16, noise, var, act, logp):
    L = lib()
    N = act.shape[0]
    if policy == "mlp64x2":
        rc = L.navppo_mlp64_act(P(flat), P(obs), D, int(f16), P(noise), N, P(var), 1, 0, None, 0, P(act), P(logp), None, _st())
    else:
        rc = L.navppo_resmlp512_act(P(flat), P(obs), int(f16), P(noise), N, P(var), 1, 0, None, 0, P(act), P(logp), None, _st())
    assert rc == 0, L.navppo_last_error().decode()


def reference_table(sim, policy, flat, quota, n_steps, fill=FILL):
    """evaluate()'s quota rule over a loop of per-step HIP launches, on the host: (flags, length, ret, path) [quota, N], count [N],
    steps [ceil(N / 16)] (the step at which the workgroup's last env met its quota, n_steps if it never did) and, per env, the step
    at which it met its quota (0 = never)."""
    N, D = sim.N, sim.D
    f16 = sim.obs_dtype == torch.float16
    io = sim.alloc_io()
    sim.reset(io.obs)
    noise = torch.zeros((N, 2), device=DEV)
    var = torch.tensor(0.5, device=DEV)   # any positive variance: the noise is zero
    act, logp = torch.empty((N, 2), device=DEV), torch.empty(N, device=DEV)
    flags = np.full((quota, N), fill, np.uint8)
    length = np.full((quota, N), fill, np.int32)
    ret = np.full((quota, N), fill, np.float32)
    path = np.full((quota, N), fill, np.float32)
    count = np.zeros(N, np.int32)
    met_at = np.zeros(N, np.int64)
    n_wg = (N + 15) // 16
    steps = np.full(n_wg, n_steps, np.int32)
    wg_open = np.ones(n_wg, bool)
    wg_of = np.arange(N) // 16
    idx = np.arange(N)
    for t in range(1, n_steps + 1):
        _act(policy, flat, io.obs, D, f16, noise, var, act, logp)
        sim.step(act, io.obs, io.reward, io.done, io.arrive, io.ended, io.ep_return, io.ep_length, ep_path=io.ep_path)
        ended, d, a = (x.cpu().numpy().astype(bool) for x in (io.ended, io.done, io.arrive))
        take = ended & (count < quota)
        f = np.where(a, 1, np.where(d, 2, 4)).astype(np.uint8)
        slot = np.minimum(count, quota - 1)
        flags[slot[take], idx[take]] = f[take]
        length[slot[take], idx[take]] = io.ep_length.cpu().numpy()[take]
        ret[slot[take], idx[take]] = io.ep_return.cpu().numpy()[take]
        path[slot[take], idx[take]] = io.ep_path.cpu().numpy()[take]
        count += take
        met_at[(count >= quota) & (met_at == 0)] = t
        for w in np.nonzero(wg_open)[0]:
            if (count[wg_of == w] >= quota).all():
                steps[w], wg_open[w] = t, False
        if not wg_open.any():
            break
    return dict(flags=flags, length=length, ret=ret, path=path, count=count, steps=steps), met_at


def kernel_table(sim, policy, flat, quota, n_steps, fill=FILL):
    """one launch through the C ABI on a fresh reset of `sim`"""
    N = sim.N
    obs0 = torch.empty((N, sim.D), dtype=sim.obs_dtype, device=DEV)
    sim.reset(obs0)
    out = dict(flags=torch.full((quota, N), fill, dtype=torch.uint8, device=DEV), length=torch.full((quota, N), fill, dtype=torch.int32, device=DEV),
               ret=torch.full((quota, N), float(fill), device=DEV), path=torch.full((quota, N), float(fill), device=DEV),
               count=torch.full((N,), -1, dtype=torch.int32, device=DEV), steps=torch.full(((N + 15) // 16,), -1, dtype=torch.int32, device=DEV))
    rc = getattr(lib(), ENTRY[policy])(sim._h, P(flat), P(obs0), quota, n_steps, P(out["flags"]), P(out["length"]), P(out["ret"]),
                                        P(out["path"]), P(out["count"]), P(out["steps"]), _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_tables_equal(got, want, what):
    for k in ("count", "steps", "flags", "length"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    for k in ("ret", "path"):   # float32 as bit patterns
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=f"{what}: {k}")


CASES = [(pol, B, f16, N, quota, m)
         for (pol, B), f16, N, quota, m in itertools.product((("mlp64x2", 10), ("mlp64x2", 36), ("resmlp512", 10)), (False, True),
                                                             (1, 16, 50, 1024), (1, 3), ("stage_1", "house_base"))]


def _case_seed(case):
    return 11 + CASES.index(case)


@functools.lru_cache(maxsize=None)
def _reference_of(case):
    pol, B, f16, N, quota, m = case
    s = _sim(N, B, f16, m, _case_seed(case))
    try:
        return reference_table(s, pol, _actor(pol, B + 6)[1], quota, quota * CAP)
    finally:
        s.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_table_equals_per_step_entry_points(case):
    """1. ep_flags / ep_length / ep_return / ep_path (bit patterns), count and steps of one persistent launch equal the table a loop
    of navppo_*_act (zero noise) + navsim_step launches yields under evaluate()'s quota rule."""
    pol, B, f16, N, quota, m = case
    want, _ = _reference_of(case)
    s = _sim(N, B, f16, m, _case_seed(case))
    try:
        got = kernel_table(s, pol, _actor(pol, B + 6)[1], quota, quota * CAP)
    finally:
        s.close()
    print(f"{case}: outcomes {np.bincount(want['flags'].reshape(-1), minlength=5)[[1, 2, 4]]} steps {want['steps'][:8]}")
    assert (want["count"] == quota).all()   # quota * cap steps always suffice
    assert_tables_equal(got, want, str(case))


def test_cases_exercise_every_outcome_and_the_early_exit():
    """The condition on the INPUTS of test 1, asserted on the reference's tables: over the cases every outcome occurs, and in
    some workgroup an env meets its quota at another step than its neighbours (it is then simulated on without being recorded,
    and workgroups leave the loop at different steps)."""
    seen, ragged, exits = set(), False, set()
    for case in CASES:
        want, met_at = _reference_of(case)
        seen |= set(np.unique(want["flags"]).tolist())
        N = case[3]
        for w in range((N + 15) // 16):
            ragged |= len(set(met_at[16 * w:16 * w + 16].tolist())) > 1
        exits |= set(want["steps"].tolist())
    assert {1, 2, 4} <= seen, seen
    assert ragged and len(exits) > 1


SENS = dict(lidar_noise_sigma=0.01, lidar_below_min="gazebo")


@pytest.mark.parametrize("pol", ["mlp64x2", "resmlp512"])
@pytest.mark.parametrize("world", ["stage_1", "house_base", "stage_1-movers", "stage_2-movers"])
def test_table_equals_per_step_entry_points_with_sensor_options(pol, world):
    """1b. The same comparison with LiDAR noise and Gazebo's below-range rule on: the SENS instantiations of evaluate_kernel /
    evaluate_resmlp_kernel (no tape; house_base: the tile-box cast) and the *_mov_kernel twins, which are always SENS (a tape of
    the mover tests, 50 envs: three full workgroups and one of 2)."""
    N, quota = 50, 2
    flat = _actor(pol, 16)[1]
    tabs = []
    for fn in (reference_table, kernel_table):
        if world.endswith("-movers"):
            from test_gpu_movers import _gpu, _phase0, _tape
            cap = 20
            s = _gpu(N, world.split("-")[0], _tape(7, 37), _phase0(7, 37, N), max_episode_steps=cap, auto_reset=True, seed=13,
                     threshold_arrive=0.4, **SENS)
            assert s.info()["step_waves"] == 8
        else:
            cap = CAP
            s = _sim(N, 10, False, world, 13, **SENS)
        try:
            r = fn(s, pol, flat, quota, quota * cap)
        finally:
            s.close()
        tabs.append(r[0] if isinstance(r, tuple) else r)
    want, got = tabs
    print(f"{pol} {world}: outcomes {np.bincount(want['flags'].reshape(-1), minlength=5)[[1, 2, 4]]} steps {want['steps']}")
    assert (want["count"] == quota).all()
    assert_tables_equal(got, want, f"{pol} {world}")


def test_n_steps_runs_out():
    """2. n_steps below one episode cap: envs still running have count < quota, unreached slots keep the caller's fill value, every
    workgroup reports n_steps -- through VecEnv.evaluate_policy on the standard evaluation env."""
    for pol in ("mlp64x2", "resmlp512"):
        flat = _actor(pol, 16)[1]
        env = VecEnv(50, map="stage_1", max_episode_steps=CAP, is_training=False, seed=3, device=DEV)
        ref = VecEnv(50, map="stage_1", max_episode_steps=CAP, is_training=False, seed=3, device=DEV)
        try:
            tab = env.evaluate_policy(flat, 2, n_steps=10, policy=pol, fill=FILL)
            want, _ = reference_table(ref.sim, pol, flat, 2, 10)
        finally:
            env.close()
            ref.close()
        got = dict(flags=tab.flags, length=tab.length, ret=tab.ret, path=tab.path, count=tab.count, steps=tab.steps)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert (want["count"] < 2).any() and (want["steps"] == 10).all()
        assert_tables_equal(got, want, pol)
        for i in range(50):   # (implied by the equality above; spelled out: the sentinel survives in every unreached slot)
            for q in range(int(got["count"][i]), 2):
                assert got["flags"][q, i] == FILL and got["length"][q, i] == FILL and got["ret"][q, i] == FILL and got["path"][q, i] == FILL


@pytest.mark.parametrize("pol,B,f16,mov", [pytest.param("mlp64x2", 10, False, None, id="mlp64x2-10-False"),
                                           pytest.param("mlp64x2", 36, True, None, id="mlp64x2-36-True"),
                                           pytest.param("resmlp512", 10, False, None, id="resmlp512-10-False"),
                                           pytest.param("mlp64x2", 10, False, 37, id="mlp64x2-10-False-movers37"),
                                           pytest.param("resmlp512", 10, False, 5, id="resmlp512-10-False-movers5"),
                                           pytest.param("mlp64x2", 10, True, 5, id="mlp64x2-10-True-movers5"),
                                           pytest.param("resmlp512", 10, False, 37, id="resmlp512-10-False-movers37")])
def test_outputs_guarded(pol, B, f16, mov):
    """3. Every argument inside a guarded allocation (tests/_guards.py), N = 50 (a ragged tail workgroup), at a 256-byte boundary
    and at the minimum alignment: guards intact, every slot written (quota * cap steps), outputs identical between placements.
    mov: with a guarded mover tape of that many segments per phase (test_gpu_tails._movers): the evaluate_*_mov_kernel twins."""
    N, quota = 50, 2
    flat = _actor(pol, B + 6)[1]

    def call(g):
        s = _sim(N, B, f16, "stage_1", 21)
        try:
            if mov:
                from test_gpu_tails import _movers
                _movers(s, g, mov)
            obs0 = g.out((N, B + 6), s.obs_dtype, 16)
            s.reset(obs0)
            pr = g.inp(flat, 16)
            fl = g.out((quota, N), torch.uint8, 1)
            ln, rt, pa = g.out((quota, N), torch.int32, 4), g.out((quota, N), torch.float32, 4), g.out((quota, N), torch.float32, 4)
            cnt, stp = g.out((N,), torch.int32, 4), g.out(((N + 15) // 16,), torch.int32, 4)
            rc = getattr(lib(), ENTRY[pol])(s._h, P(pr), P(obs0), quota, quota * CAP, P(fl), P(ln), P(rt), P(pa), P(cnt), P(stp), _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            assert bool((cnt == quota).all())
            return fl
        finally:
            s.close()

    run_both(DEV, call, f"{ENTRY[pol]} B={B} f16={f16} movers={mov}")


def _save_actor(policy, tmp_path):
    actor, _ = _actor(policy, 16, seed=9)
    d = tmp_path / "m" / "checkpoints"
    d.mkdir(parents=True, exist_ok=True)
    path = str(d / "actor_iter0001_step00000100.pth")
    torch.save({k: v.detach().cpu().clone() for k, v in actor.state_dict().items()}, path)
    return path


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_evaluate_persistent(policy, tmp_path):
    """5. evaluate(persistent=True) on a saved random-init checkpoint: its rows equal those of a per-step HIP loop under evaluate()'s
    ordering (slot-major, cut to num_episodes); CSV header and summary keys are those of persistent=False; episodes == num_episodes
    when num_episodes is not a multiple of n_parallel."""
    path = _save_actor(policy, tmp_path)
    assert ev.find_latest_checkpoint(str(tmp_path), "m") == path
    actor, pol = ev.load_actor(path, DEV)
    assert pol == policy
    n_ep, n_par, cap = 40, 16, 25
    kw = dict(num_episodes=n_ep, max_timesteps_per_episode=cap, n_parallel=n_par, seed=4, log=None)
    lines = []
    sp = ev.evaluate(actor, output_dir=str(tmp_path / "p"), method_name="m", persistent=True, **dict(kw, log=lines.append))
    sl = ev.evaluate(actor, output_dir=str(tmp_path / "l"), method_name="m", **kw)
    assert sp["episodes"] == n_ep == len(sp["rows"]) and set(sp) == set(sl)
    assert len(lines) == 1 and lines[0].startswith("EVALUATION SUMMARY")
    hp, hl = (next(csv.reader(open(s["csv"]))) for s in (sp, sl))
    assert hp == hl == ["episode", "success", "collision", "timeout", "length", "return", "path_length", "time"]
    assert len(list(csv.reader(open(sp["csv"])))) == n_ep + 1
    # the per-step HIP loop on the same env (evaluate()'s VecEnv: stage_1, arrival threshold 0.4, seed)
    quota = -(-n_ep // n_par)
    ref = VecEnv(n_par, map="stage_1", max_episode_steps=cap, auto_reset=True, is_training=False, seed=4, device=DEV)
    try:
        want, _ = reference_table(ref.sim, policy, nets.flat_actor_params(actor).to(DEV), quota, quota * cap)
    finally:
        ref.close()
    f = want["flags"].reshape(-1)[:n_ep]
    rows = [[k, int(f[k] & 1), int(f[k] >> 1 & 1), int(f[k] >> 2 & 1), int(want["length"].reshape(-1)[k]),
             float(want["ret"].reshape(-1)[k]), float(want["path"].reshape(-1)[k])] for k in range(n_ep)]
    assert [r[:7] for r in sp["rows"]] == rows
    assert all(r[7] > 0 for r in sp["rows"])


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_eval_during_training_does_not_perturb_training(policy, tmp_path):
    """6. Two trainers, same seed, 3 iterations, eval_every = 1 against 0: flat parameters, Adam moments and the last rollout's
    buffers bit-identical; the first has three rows in <method>_eval_history.csv and eval_* figures, the second neither."""
    res = {}
    for every in (1, 0):
        env = VecEnv(64, map="stage_1", max_episode_steps=30, seed=2, device=DEV)
        out = tmp_path / f"e{every}"
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=32, max_episode_steps=30, n_updates_per_iteration=2, policy=policy, seed=1,
                                               eval_every=every, eval_episodes=20, output_dir=str(out), method_name="m"))
        seen = []
        for _ in range(3):
            tr.iteration()
            seen.append({k for k in tr.stats if k.startswith("eval_")})
        torch.cuda.synchronize()
        assert tr.updater.fused
        res[every] = [t.clone() for t in (tr.updater.fp.flat, tr.updater._adam_m, tr.updater._adam_v, tr.obs_buf, tr.act_buf,
                                          tr.logp_buf, tr.rew_buf, tr.ended_buf, tr.rtg_buf, tr._step_base)]
        hist = out / "m" / "logs" / "m_eval_history.csv"
        if every:
            assert all({"eval_success", "eval_collision", "eval_timeout", "eval_return", "eval_length"} <= s for s in seen)
            rows = list(csv.reader(open(hist)))
            assert rows[0] == ["iteration", "timesteps", "episodes", "success_rate", "collision_rate", "timeout_rate", "mean_length",
                               "mean_return", "mean_path_length"]
            assert [r[0] for r in rows[1:]] == ["1", "2", "3"] and all(r[2] == "20" for r in rows[1:])
            lg = tr.stats
            assert abs(lg["eval_success"] + lg["eval_collision"] + lg["eval_timeout"] - 1.0) < 1e-12
            assert tr._eval_env.N == 20 and tr._eval_env.threshold_arrive == 0.4
        else:
            assert not any(seen) and not os.path.exists(hist) and getattr(tr, "_eval_env", None) is None
        if getattr(tr, "_eval_env", None) is not None:
            tr._eval_env.close()
        env.close()
    for a, b in zip(res[1], res[0]):
        assert torch.equal(a, b)


def test_argument_errors_launch_nothing():
    """7. Each refused call returns NAVSIM_E_ARG with a message and leaves the output buffers as they were."""
    L = lib()
    f64, f512 = _actor("mlp64x2", 16)[1], _actor("resmlp512", 16)[1]
    f42 = _actor("mlp64x2", 42)[1]

    def attempt(sim, entry, flat, quota, n_steps, word):
        N = sim.N
        obs0 = torch.zeros((N, sim.D), dtype=sim.obs_dtype, device=DEV)
        q = max(quota, 1)
        outs = [torch.full((q, N), FILL, dtype=torch.uint8, device=DEV), torch.full((q, N), FILL, dtype=torch.int32, device=DEV),
                torch.full((q, N), float(FILL), device=DEV), torch.full((q, N), float(FILL), device=DEV),
                torch.full((N,), FILL, dtype=torch.int32, device=DEV), torch.full(((N + 15) // 16,), FILL, dtype=torch.int32, device=DEV)]
        rc = getattr(L, entry)(sim._h, P(flat), P(obs0), quota, n_steps, *[P(o) for o in outs], _st())
        msg = L.navsim_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and entry in msg and word in msg, (rc, msg)
        assert all(bool((o == FILL).all()) for o in outs), msg

    for entry, flat in (("navsim_evaluate_mlp64", f64), ("navsim_evaluate_resmlp512", f512)):
        s = _sim(50, 10, False, "stage_1", 1)
        attempt(s, entry, flat, 0, 10, "quota")
        attempt(s, entry, flat, 1, 0, "n_steps")
        s.close()
        s = _sim(50, 10, False, "stage_1", 1, auto_reset=False)
        attempt(s, entry, flat, 1, 10, "auto_reset")
        s.close()
        s = _sim(50, 10, False, "stage_1", 1, cap=0)
        attempt(s, entry, flat, 1, 10, "max_episode_steps")
        s.close()
        s = _sim(4097, 10, False, "stage_1", 1)
        attempt(s, entry, flat, 1, 10, "4096")
        s.close()
    s = _sim(50, 36, False, "stage_1", 1)
    attempt(s, "navsim_evaluate_resmlp512", f512, 1, 10, "10 beams")
    torch.cuda.synchronize()
    s.close()
    # ... and the Python surface refuses the same without a fallback
    env = VecEnv(16, map="stage_1", n_beams=36, max_episode_steps=CAP, is_training=False, device=DEV)
    with pytest.raises(ValueError, match="no evaluation kernel"):
        env.evaluate_policy(f512, 1, policy="resmlp512")
    tab = env.evaluate_policy(f42, 1, policy="mlp64x2")
    assert int(tab.count.min()) == 1
    env.close()
