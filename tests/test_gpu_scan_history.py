"""Scan history on the GPU: navsim_stack_rows, navsim_rollout_mlp64_hist, navsim_evaluate_mlp64_hist, HistoryWindow and
PPOConfig.scan_history.

Nothing is recomputed anywhere in the feature -- a history row is 38 copies -- so every comparison is bit for bit.  The reference
of the two persistent kernels is written HERE from the per-step entry points: navsim_reset, then per step HistoryWindow
(navsim_stack_rows on the last three rows) -> navppo_mlp64_act (obs_dim = 42, the same seed / env_id_base / step_base) -> navsim_step.

The common world: 40 envs (two full 16-env workgroups and one of 8), 48 steps, episodes capped at 7 steps and -- set_state behind the
reset -- started at step count env mod 7, so that time-outs fall on row 0, on row 1 and on consecutive rows of neighbouring envs; the
robot starts 0.24 m in front of stage_2's inner wall with goals drawn in a 1 m box next to it (arrival threshold 0.4), so that
collisions and arrivals end episodes one or two steps after a reset.

Beside the bit-for-bit comparisons one check stands on its own feet (4b): the rollout kernel's actions and log-probs against a float64
actor on stack_rows_reference rows of the kernel's own observation buffer, with the draws of tests/_noise.py.  Placement (2b): an env's
trajectory depends on its global id alone -- one handle against two shards, the id carry inside a workgroup, a grid beyond one round
of workgroups.  The trainer (8): the update consumes exactly the rows the rule prescribes, under every update option."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _noise
from _guards import run_both
from navbot_ppo_amd import evaluate as ev, maps, nets, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import HIST_DIM, HistoryWindow, NavSim, NavsimError, VecEnv, stack_rows, stack_rows_reference
from oracle import navsim_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, T, CAP = 40, 48, 7
ACT_SEED, STEP_BASE, VAR = 0x5EED1234ABCD, 5, 0.3
WORLD = dict(n_beams=10, max_episode_steps=CAP, auto_reset=True, threshold_arrive=0.4, spawn=(0.8, 1.66, math.pi / 2),
             goal_box=(0.6, 1.6))


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(x):
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _actor(seed=3, scale=2.0):
    """a random 42-64-64 actor with every column's weights non-zero, and its flat parameters"""
    torch.manual_seed(seed)
    a, _ = nets.make_policy("mlp64x2", HIST_DIM)
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(scale)
    assert bool((a.layer1.weight != 0).all())
    a = a.to(DEV)
    return a, nets.flat_actor_params(a).to(DEV)


# ---------------------------------------------------------------- the worlds of the closed-loop cases
def _bank3():
    return maps.mover_bank([maps.movers_by_name("orbit4", 8), maps.movers_by_name("patrol2", 5), maps.movers_by_name("orbit2", 13)])


KINDS = {   # name -> (map, NavSim options, movers)
    "plain": ("stage_2", {}, None),
    "noise-gazebo": ("stage_2", dict(lidar_noise_sigma=0.02, lidar_below_min="gazebo"), None),
    "f16": ("stage_2", dict(obs_f16=True), None),
    "stage_1": ("stage_1", {}, None),             # 32 segments: the cast without tile boxes
    "house-boxes": ("house_base", {}, None),      # 256 segments, the curated start / goal tables of the house
    "orbit4": ("stage_1", {}, "orbit4"),
    "orbit4-boxes": ("stage_2", {}, "orbit4"),
    "bank3-respawn": ("stage_2", dict(respawn_on_arrive=True), "bank3"),
    # the kMovSens instantiations with the sensor options on, float16 rows under them, per-env maps, and the episode rules off
    "orbit4-noise-gazebo": ("stage_1", dict(lidar_noise_sigma=0.02, lidar_below_min="gazebo"), "orbit4"),
    "bank3-noise-f16": ("stage_2", dict(respawn_on_arrive=True, lidar_noise_sigma=0.02, obs_f16=True), "bank3"),
    "noise-f16": ("stage_2", dict(lidar_noise_sigma=0.02, lidar_below_min="gazebo", obs_f16=True), None),
    "per-env": ("stage_2:per-env", {}, None),     # every env its own jittered, re-ordered copy of the 128 segments
    "no-reset": ("stage_2", dict(auto_reset=False), None),   # an ended env keeps its row: hist_next_entry's sm.obs branch on a cut
    "no-reset-respawn": ("stage_2", dict(auto_reset=False, respawn_on_arrive=True), None),
    "no-cap": ("stage_2", dict(max_episode_steps=0), None),  # collisions and arrivals alone end episodes
}


def world_of(kind):
    return {**WORLD, **KINDS[kind][1]}


def make_sim(kind, n=N, seed=11, env_id_base=0):
    """the world `kind` for the envs env_id_base .. env_id_base + n - 1: mover phases and tape ids follow the global env id"""
    m, _, movers = KINDS[kind]
    m, _, per_env = m.partition(":")
    w = world_of(kind)
    if m == "house_base":
        w = {k: v for k, v in w.items() if k not in ("spawn", "goal_box")}
        s = NavSim(n, seed=seed, env_id_base=env_id_base, device=DEV, **w)
        s.set_map(maps.by_name(m))
        s.set_spawn_sampler(*maps.spawn_tables("small_house", min_dist=0.3, max_dist=6.0))
    else:
        s = NavSim(n, seed=seed, env_id_base=env_id_base, device=DEV, **w)
        rr, rs = maps.goal_rects(m)
        s.set_goal_rects(0, rr)
        s.set_goal_rects(1, rs)
        seg = maps.by_name(m)
        s.set_map(maps.replicate_per_env(seg, n, seed=0) if per_env else seg)
    if movers == "orbit4":
        tape = maps.movers_by_name("orbit4", 16)
        s.set_movers(tape, maps.mover_phases(tape.shape[0], n, map_seed=2, env_id_base=env_id_base))
    elif movers == "bank3":
        bank, periods, _ = _bank3()
        ids = maps.mover_tape_ids(3, n, map_seed=2, env_id_base=env_id_base)
        s.set_mover_bank(bank, periods, ids, maps.mover_bank_phases(periods[ids], map_seed=2, env_id_base=env_id_base))
    return s


def start(sim, obs0):
    """the start of every closed-loop case: a reset, then staggered step counts (the env with global id g has taken g mod 7 steps of
    its episode)"""
    sim.reset(obs0)
    sim.set_state(ep_step=((int(sim.cfg.env_id_base) + np.arange(sim.N)) % CAP).astype(np.int32))


def _buffers(sim, n_steps):
    n = sim.N
    z = lambda dt, *s: torch.zeros((n_steps, n) + s, dtype=dt, device=DEV)
    return dict(obs=torch.zeros((n_steps + 1, n, 16), dtype=sim.obs_dtype, device=DEV), act=z(torch.float32, 2), logp=z(torch.float32),
                reward=z(torch.float32), done=z(torch.uint8), arrive=z(torch.uint8), ended=z(torch.uint8), ep_return=z(torch.float32),
                ep_length=z(torch.int32), ep_path=z(torch.float32))


FIELDS = ("obs", "act", "logp", "reward", "done", "arrive", "ended", "ep_return", "ep_length", "ep_path")


def kernel_rollout(sim, flat, n_steps, b=None):
    """navsim_rollout_mlp64_hist through the C ABI from start(); returns the buffers and the handle's state afterwards"""
    b = _buffers(sim, n_steps) if b is None else b
    start(sim, b["obs"][0])
    var = torch.tensor(VAR, device=DEV)
    base = torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
    rc = lib().navsim_rollout_mlp64_hist(sim._h, P(flat), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                                         P(b["arrive"]), P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var),
                                         ACT_SEED, P(base), n_steps, _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()
    return b, sim.get_state()


def stepping_rollout(sim, flat, n_steps):
    """the same rollout from the per-step entry points: HistoryWindow -> navppo_mlp64_act(obs_dim = 42) -> navsim_step"""
    L = lib()
    b = _buffers(sim, n_steps)
    start(sim, b["obs"][0])
    var = torch.tensor(VAR, device=DEV)
    base = torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
    f16 = int(sim.obs_dtype == torch.float16)
    win = HistoryWindow(sim.N, DEV, sim.obs_dtype)
    row = win.reset(b["obs"][0])
    hist = [row.clone()]
    for t in range(n_steps):
        rc = L.navppo_mlp64_act(P(flat), P(row), HIST_DIM, f16, None, sim.N, P(var), ACT_SEED, int(sim.cfg.env_id_base), P(base), t,
                                P(b["act"][t]), P(b["logp"][t]), None, _st())
        assert rc == 0, L.navppo_last_error().decode()
        sim.step(b["act"][t], b["obs"][t + 1], b["reward"][t], b["done"][t], b["arrive"][t], b["ended"][t], b["ep_return"][t],
                 b["ep_length"][t], ep_path=b["ep_path"][t])
        row = win.push(b["obs"][t + 1], b["ended"][t])
        hist.append(row.clone())
    torch.cuda.synchronize()
    b["hist"] = torch.stack(hist)
    return b, sim.get_state()


@functools.lru_cache(maxsize=None)
def _stepping_of(kind, n=N, n_steps=T, env_id_base=0):
    s = make_sim(kind, n, env_id_base=env_id_base)
    try:
        return stepping_rollout(s, _actor()[1], n_steps)
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def _kernel_of(kind, n=N, n_steps=T, env_id_base=0):
    s = make_sim(kind, n, env_id_base=env_id_base)
    try:
        return kernel_rollout(s, _actor()[1], n_steps)
    finally:
        s.close()


def assert_cuts_cover_the_edges(ended):
    """what a case must hold before it is used: for some env a cut on row 0 or 1, and for some env two cuts less than three rows
    apart (ended[t] set makes row t + 1 an episode start; row 0 always is one)"""
    e = ended.cpu().numpy() != 0
    assert e[:2].any(), "no env has a cut on row 0 or 1"
    close = (e[:-1] & e[1:]).any() or (e[:-2] & e[2:]).any()
    assert close, "no env has two cuts less than three rows apart"


def longest_run(ended):
    """the longest run of consecutive rows with `ended` set, over all envs"""
    e = ended.cpu().numpy() != 0
    run, best = np.zeros(e.shape[1], np.int64), 0
    for t in range(e.shape[0]):
        run = np.where(e[t], run + 1, 0)
        best = max(best, int(run.max()))
    return best


def cut_facts(b):
    """the figures a closed-loop case prints: how often the stepping loop (the reference) cut, and where"""
    e = b["ended"].cpu().numpy() != 0
    close = (e[:-1] & e[1:]).sum() + (e[:-2] & e[2:]).sum() if e.shape[0] > 2 else 0
    return (f"ended {int(e.sum())} done {int(b['done'].sum())} arrive {int(b['arrive'].sum())}; cuts on rows 0-1: {int(e[:2].sum())}, "
            f"pairs of cuts less than three rows apart: {int(close)}, longest run of ended rows: {longest_run(b['ended'])}")


def assert_the_world_exercises_the_cuts(kind, b):
    """Conditions on the stepping loop's rollout, per world.  auto_reset: assert_cuts_cover_the_edges.  Without it an env that timed
    out or collided keeps ending (its step count stays past the cap, it stays at the wall): some env must have three consecutive
    ended rows, so that rows start an episode back to back from the row the step left.  Without a cap: a collision or an arrival
    must cut, there is nothing else that does."""
    w = world_of(kind)
    if w["auto_reset"]:
        assert_cuts_cover_the_edges(b["ended"])
    else:
        assert longest_run(b["ended"]) >= 3, "no env has three consecutive ended rows"
    if w["max_episode_steps"] == 0:
        assert int(((b["done"] != 0) | (b["arrive"] != 0)).sum()) >= 1, "no collision or arrival cut"


def assert_same_rollout(got, got_state, want, want_state, what):
    for f in FIELDS:
        assert same(got[f], want[f]), f"{what}: {f} (first differing row "  \
            f"{int((bits(got[f]).reshape(got[f].shape[0], -1) != bits(want[f]).reshape(want[f].shape[0], -1)).any(1).nonzero()[0])})"
    for k in want_state:
        assert np.array_equal(got_state[k], want_state[k]), f"{what}: state {k}"


# ---------------------------------------------------------------- 1. navsim_stack_rows against the reference
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("R,n", [(1, 1), (2, 37), (49, 40), (3, 4099)])
def test_stack_rows_equals_the_reference(R, n, f16):
    rng = np.random.default_rng(1000 * R + n)
    obs = rng.standard_normal((R, n, 16)).astype(np.float16 if f16 else np.float32)
    for density in (0.0, 0.3, 1.0):
        ended = (rng.random((max(R - 1, 0), n)) < density).astype(np.uint8)
        want = stack_rows_reference(obs, ended if R > 1 else None)
        o, e = torch.from_numpy(obs).to(DEV), torch.from_numpy(ended).to(DEV)

        def call(g):
            oo = g.inp(o, 16)
            ee = g.inp(e, 1) if R > 1 else None
            out = g.out((R, n, HIST_DIM), o.dtype, 16)
            rc = lib().navsim_stack_rows(P(oo), int(f16), P(ee), R, n, P(out), _st())
            assert rc == 0, lib().navsim_last_error().decode()
            return out

        got = run_both(DEV, call, f"navsim_stack_rows R={R} N={n} f16={f16} density={density}")
        assert same(got, torch.from_numpy(want).to(DEV)), (R, n, f16, density)
        assert same(stack_rows(o, e if R > 1 else None), got)   # the wrapper, on ordinary allocations


def test_history_window_is_the_last_row_of_the_full_stack():
    b, _ = _stepping_of("plain")
    full = stack_rows(b["obs"], b["ended"])
    assert same(b["hist"], full)
    assert same(full.cpu(), torch.from_numpy(stack_rows_reference(b["obs"].cpu().numpy(), b["ended"].cpu().numpy())))


# ---------------------------------------------------------------- 2. the rollout kernel against the stepping loop
# 4117 envs: 258 workgroups -- more than the 256 CUs hold at once, so the grid runs in rounds -- the last one with 5 envs
N_BIG, T_BIG = 4117, 12
ROLLOUT_CASES = [(k, N, T) for k in KINDS] + [("plain", 5, T), ("plain", N, 1), ("bank3-respawn", 5, 3)]  \
    + [("plain", N_BIG, T_BIG), ("orbit4", N_BIG, T_BIG)]


@pytest.mark.parametrize("kind,n,n_steps", ROLLOUT_CASES, ids=lambda v: str(v))
def test_rollout_hist_equals_the_stepping_loop(kind, n, n_steps):
    want, want_state = _stepping_of(kind, n, n_steps)
    print(f"{kind} N={n} T={n_steps}: {cut_facts(want)}")
    if (n, n_steps) in ((N, T), (N_BIG, T_BIG)):
        assert_the_world_exercises_the_cuts(kind, want)
    got, got_state = _kernel_of(kind, n, n_steps)
    assert_same_rollout(got, got_state, want, want_state, kind)


# ---------------------------------------------------------------- 2b. placement and keys
SHARDS = ((0, 24), (24, 16))   # (env_id_base, envs): env 24 is lane 8 of workgroup 1 in the whole run, lane 0 of workgroup 0 in its shard


@pytest.mark.parametrize("kind", ["plain", "bank3-noise-f16"])
def test_rollout_hist_does_not_depend_on_the_placement(kind):
    """One handle of 40 envs against two of 24 and 16 with env_id_base 0 and 24, the same seeds: an env's trajectory depends on its
    global id alone, not on the lane or the workgroup that holds it (the `hist` block in LDS is indexed by the local env)."""
    whole, whole_state = _kernel_of(kind)
    parts = [_kernel_of(kind, n, T, base) for base, n in SHARDS]
    assert not same(parts[1][0]["act"], whole["act"][:, :16])   # (the second shard is not the first 16 envs again)
    for f in FIELDS:
        assert same(torch.cat([p[0][f] for p in parts], dim=1), whole[f]), f"{kind}: {f}"
    for k in whole_state:
        assert np.array_equal(np.concatenate([p[1][k] for p in parts]), whole_state[k]), f"{kind}: state {k}"


def test_rollout_hist_with_the_env_id_carry_inside_a_workgroup():
    """env_id_base = 2^32 - 20: envs 20 .. 39 have counter word 1 = 1, the carry falls inside workgroup 1 (envs 16 .. 31)"""
    base = (1 << 32) - 20
    want, want_state = _stepping_of("plain", N, T, base)
    print(f"plain env_id_base=2^32-20: {cut_facts(want)}")
    assert_the_world_exercises_the_cuts("plain", want)
    got, got_state = _kernel_of("plain", N, T, base)
    assert_same_rollout(got, got_state, want, want_state, "plain, env_id_base = 2^32 - 20")
    assert not same(got["act"], _kernel_of("plain")[0]["act"])


def test_rollout_hist_of_zero_steps_touches_nothing():
    s = make_sim("plain")
    try:
        b = _buffers(s, T)
        for f in FIELDS:
            b[f].fill_(7)
        start(s, b["obs"][0])
        torch.cuda.synchronize()
        before, state = {f: b[f].clone() for f in FIELDS}, s.get_state()
        var = torch.tensor(VAR, device=DEV)
        base = torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
        rc = lib().navsim_rollout_mlp64_hist(s._h, P(_actor()[1]), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                                             P(b["arrive"]), P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var),
                                             ACT_SEED, P(base), 0, _st())
        assert rc == 0, lib().navsim_last_error().decode()
        torch.cuda.synchronize()
        after = s.get_state()
    finally:
        s.close()
    for f in FIELDS:
        assert same(b[f], before[f]), f
    for k in state:
        assert np.array_equal(after[k], state[k]), k


# ---------------------------------------------------------------- 3. the env side is untouched
@pytest.mark.parametrize("kind", ["plain", "f16", "bank3-respawn"])
def test_env_side_replays_on_step_seq(kind):
    got, got_state = _kernel_of(kind)
    s = make_sim(kind)
    try:
        obs0 = torch.zeros((N, 16), dtype=s.obs_dtype, device=DEV)
        start(s, obs0)
        b = _buffers(s, T)
        s.step_seq(got["act"], b["obs"][1:], b["reward"], b["done"], b["arrive"], b["ended"], b["ep_return"], b["ep_length"], b["ep_path"])
        torch.cuda.synchronize()
        state = s.get_state()
    finally:
        s.close()
    assert same(obs0, got["obs"][0])
    for f in ("reward", "done", "arrive", "ended", "ep_return", "ep_length", "ep_path"):
        assert same(b[f], got[f]), f
    assert same(b["obs"][1:], got["obs"][1:])
    for k in state:
        assert np.array_equal(state[k], got_state[k]), k


def test_env_side_replays_on_the_oracle():
    """the recorded actions on the CPU oracle: flags exactly, observations to the 1e-6 the step kernels are held to against it"""
    got, _ = _kernel_of("plain")
    rr, rs = maps.goal_rects("stage_2")
    cpu = O.OracleSim(N, seed=11, **WORLD)
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    cpu.set_map(maps.by_name("stage_2"))
    obs = got["obs"].cpu().numpy()
    acts = got["act"].cpu().numpy()
    np.testing.assert_allclose(obs[0], cpu.reset(), rtol=0, atol=1e-6)
    cpu.set_state(ep_step=(np.arange(N) % CAP).astype(np.int32))
    exact = 0
    for t in range(T):
        out = cpu.step(acts[t])
        for f in ("done", "arrive", "ended"):
            np.testing.assert_array_equal(got[f][t].cpu().numpy(), out[f], err_msg=f"{f}, step {t}")
        np.testing.assert_allclose(obs[t + 1], out["obs"], rtol=0, atol=1e-6, err_msg=f"obs, step {t}")
        exact += int((obs[t + 1] == out["obs"]).all(axis=1).sum())
    assert exact > 0.99 * T * N


# ---------------------------------------------------------------- 4. the history is really read
def test_the_two_older_frames_are_read():
    """Two actors that differ only in columns 16..35: the second has the weights of the two older scan blocks swapped.  On row 0 both
    older frames are copies of the row's scan, so the two actors see the same sums in another order: equal to float32 resolution.
    From the first row on which the two older frames differ (row 2 of an episode) the actions differ."""
    a, flat = _actor()
    W = a.layer1.weight.detach().clone()
    W2 = W.clone()
    W2[:, 16:26], W2[:, 26:36] = W[:, 26:36], W[:, 16:26]
    flat2 = flat.clone()
    flat2[:64 * HIST_DIM] = W2.reshape(-1)
    assert bool((flat2 != flat).any()) and same(flat2[64 * HIST_DIM:], flat[64 * HIST_DIM:])
    outs = []
    for f in (flat, flat2):
        s = NavSim(N, seed=4, device=DEV, n_beams=10, max_episode_steps=40, auto_reset=True)   # long episodes from the map's centre
        try:
            s.set_map(maps.by_name("stage_1"))
            b = _buffers(s, 6)
            s.reset(b["obs"][0])
            var = torch.tensor(VAR, device=DEV)
            rc = lib().navsim_rollout_mlp64_hist(s._h, P(f), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                                                 P(b["arrive"]), P(b["ended"]), None, None, None, P(var), ACT_SEED, None, 6, _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            outs.append(b)
        finally:
            s.close()
    x, y = outs
    assert same(x["obs"][0], y["obs"][0])
    # the envs whose rows 0..2 lie in one episode under both actors (a goal drawn next to the start ends an episode at once)
    keep = ((x["ended"][:2] == 0) & (y["ended"][:2] == 0)).all(0)
    assert int(keep.sum()) >= N // 2
    # row 0: the pre-activations agree to summation order; the heads are sigmoid / tanh (slope <= 1) of sums of 64 terms of size O(1),
    # so the actions agree to a few hundred float32 ulps of 1 at the most
    assert torch.allclose(x["act"][0], y["act"][0], rtol=0, atol=512 * 2.0 ** -24)
    assert not torch.equal(x["act"][2][keep], y["act"][2][keep])
    assert float((x["act"][2][keep] - y["act"][2][keep]).abs().max()) > 1e-3


# ---------------------------------------------------------------- 4b. the rollout kernel against a float64 actor, closed loop
REL = 16 * 2.0 ** -24       # a draw against the float64 Philox / Box-Muller reference, per max(1, rad): test_gpu_action_noise.REL
LOG_2PI = 1.8378770664093453


@functools.lru_cache(maxsize=None)
def _host_actors():
    """the actor of the closed-loop cases as torch's float32 module on the host, and its float64 copy"""
    a = copy.deepcopy(_actor()[0]).cpu()
    return a, copy.deepcopy(a).double()


def closed_loop_ratios(kind, swap_older_frames=False):
    """Every action and log-prob of the cached kernel rollout `kind` against a reference that runs no kernel of the project: the rows
    are stack_rows_reference of the kernel's own obs / ended buffers, the mean is the float64 actor on them (float16 rows widen
    exactly), the draws are tests/_noise.py's.  expected action = clamp(mean64 + sqrt(var) e), var the float32 the kernel is handed.
    Bound per entry, from what the project already asserts elsewhere:
        |mean32 - mean64|              torch's float32 actor against its float64 copy on the same rows: a reference-only quantity
      + 1e-5 |mean64| + 2e-6           navppo_mlp64_act against torch's float32 actor (test_fused_act_and_value_on_wide_and_half_rows)
      + sqrt(var) REL max(1, rad)      the draws (test_gpu_action_noise.REL)
    and the clamp is 1-Lipschitz, so no entry is left out.  logp: the float64 formula on the kernel's own action and mean64 at
    check_logp's rtol 1e-4, atol 2e-5, plus what the mean's bound m moves the formula by: sum_j (|a_j - mean_j| m_j + m_j^2 / 2) / var.
    Returns (error / bound of the actions [T, N, 2], of logp [T, N], steps into the episode of every row [T, N])."""
    b, _ = _kernel_of(kind)
    obs, ended = b["obs"].cpu().numpy(), b["ended"].cpu().numpy()
    rows = stack_rows_reference(obs, ended)[:T]
    if swap_older_frames:
        sw = rows.copy()
        sw[..., 16:26], sw[..., 26:36] = rows[..., 26:36], rows[..., 16:26]
        rows = sw
    a32, a64 = _host_actors()
    x = torch.from_numpy(rows.astype(np.float32).reshape(T * N, HIST_DIM))
    with torch.no_grad():
        m32, m64 = a32(x).double().numpy(), a64(x.double()).numpy()
    var = float(np.float32(VAR))
    sd = math.sqrt(var)
    e, rad = np.empty((T, N, 2)), np.empty((T, N))
    for t in range(T):
        _, u1, _, e[t, :, 0], e[t, :, 1] = _noise.action_noise(ACT_SEED, list(range(N)), STEP_BASE + t)
        rad[t] = _noise.rad_of(u1)
    raw = m64 + sd * e.reshape(T * N, 2)
    want = np.stack([raw[:, 0].clip(0.0, 1.0), raw[:, 1].clip(-1.0, 1.0)], 1)
    m_bound = np.abs(m32 - m64) + 1e-5 * np.abs(m64) + 2e-6
    bound = m_bound + sd * REL * np.maximum(1.0, rad).reshape(T * N, 1)
    act = b["act"].cpu().numpy().astype(np.float64).reshape(T * N, 2)
    r_act = np.abs(act - want) / bound
    lp_want = -0.5 * ((act - m64) ** 2).sum(1) / var - LOG_2PI - math.log(var)
    lp_bound = 2e-5 + 1e-4 * np.abs(lp_want) + ((np.abs(act - m64) * m_bound + 0.5 * m_bound ** 2).sum(1)) / var
    r_lp = np.abs(b["logp"].cpu().numpy().astype(np.float64).reshape(-1) - lp_want) / lp_bound
    first = np.zeros(N, np.int64)   # r(t) of stack_rows_reference
    depth = np.empty((T, N), np.int64)
    for t in range(T):
        if t > 0:
            first = np.where(ended[t - 1] != 0, t, first)
        depth[t] = t - first
    return r_act.reshape(T, N, 2), r_lp.reshape(T, N), depth


@pytest.mark.parametrize("kind", ["plain", "f16", "bank3-respawn"])
def test_rollout_hist_against_a_float64_actor_on_reference_rows(kind):
    r_act, r_lp, depth = closed_loop_ratios(kind)
    print(f"{kind}: worst error / bound: actions {r_act.max():.3f}, logp {r_lp.max():.3f}")
    assert (r_act <= 1.0).all(), (kind, float(r_act.max()), np.argwhere(r_act > 1.0)[:4].tolist())
    assert (r_lp <= 1.0).all(), (kind, float(r_lp.max()), np.argwhere(r_lp > 1.0)[:4].tolist())
    # the check sees the order of the two older frames: with them swapped in the reference rows it fails on most rows on which
    # they can differ (rows at least two steps into an episode; on every other row both are the same scan)
    s_act, _, _ = closed_loop_ratios(kind, swap_older_frames=True)
    deep = depth >= 2
    failed = (s_act > 1.0).any(-1)
    print(f"{kind}: rows at least two steps into an episode {int(deep.sum())}, of which the swapped check fails {int((failed & deep).sum())}")
    assert int(deep.sum()) >= N
    assert int((failed & deep).sum()) > int(deep.sum()) // 2
    assert not failed[depth == 0].any()   # (an episode's first row holds its own scan three times)


# ---------------------------------------------------------------- 5. the evaluation kernel
def reference_table_hist(sim, flat, quota, n_steps, fill=77):
    """evaluate()'s quota rule (tests/test_gpu_evaluate.reference_table) over the stepping loop with zero noise"""
    n = sim.N
    f16 = int(sim.obs_dtype == torch.float16)
    io = sim.alloc_io()
    sim.reset(io.obs)
    win = HistoryWindow(n, DEV, sim.obs_dtype)
    row = win.reset(io.obs)
    noise = torch.zeros((n, 2), device=DEV)
    var = torch.tensor(0.5, device=DEV)
    act, logp = torch.empty((n, 2), device=DEV), torch.empty(n, device=DEV)
    flags, length = np.full((quota, n), fill, np.uint8), np.full((quota, n), fill, np.int32)
    ret, path = np.full((quota, n), fill, np.float32), np.full((quota, n), fill, np.float32)
    count = np.zeros(n, np.int32)
    n_wg = (n + 15) // 16
    steps, wg_open, wg_of, idx = np.full(n_wg, n_steps, np.int32), np.ones(n_wg, bool), np.arange(n) // 16, np.arange(n)
    for t in range(1, n_steps + 1):
        rc = lib().navppo_mlp64_act(P(flat), P(row), HIST_DIM, f16, P(noise), n, P(var), 1, 0, None, 0, P(act), P(logp), None, _st())
        assert rc == 0, lib().navppo_last_error().decode()
        sim.step(act, io.obs, io.reward, io.done, io.arrive, io.ended, io.ep_return, io.ep_length, ep_path=io.ep_path)
        row = win.push(io.obs, io.ended)
        ended, d, a = (x.cpu().numpy().astype(bool) for x in (io.ended, io.done, io.arrive))
        take = ended & (count < quota)
        f = np.where(a, 1, np.where(d, 2, 4)).astype(np.uint8)
        slot = np.minimum(count, quota - 1)
        flags[slot[take], idx[take]] = f[take]
        length[slot[take], idx[take]] = io.ep_length.cpu().numpy()[take]
        ret[slot[take], idx[take]] = io.ep_return.cpu().numpy()[take]
        path[slot[take], idx[take]] = io.ep_path.cpu().numpy()[take]
        count += take
        for w in np.nonzero(wg_open)[0]:
            if (count[wg_of == w] >= quota).all():
                steps[w], wg_open[w] = t, False
        if not wg_open.any():
            break
    return dict(flags=flags, length=length, ret=ret, path=path, count=count, steps=steps)


def kernel_table_hist(sim, flat, quota, n_steps, fill=77):
    n = sim.N
    obs0 = torch.empty((n, 16), dtype=sim.obs_dtype, device=DEV)
    sim.reset(obs0)
    out = dict(flags=torch.full((quota, n), fill, dtype=torch.uint8, device=DEV), length=torch.full((quota, n), fill, dtype=torch.int32, device=DEV),
               ret=torch.full((quota, n), float(fill), device=DEV), path=torch.full((quota, n), float(fill), device=DEV),
               count=torch.full((n,), -1, dtype=torch.int32, device=DEV), steps=torch.full(((n + 15) // 16,), -1, dtype=torch.int32, device=DEV))
    rc = lib().navsim_evaluate_mlp64_hist(sim._h, P(flat), P(obs0), quota, n_steps, P(out["flags"]), P(out["length"]), P(out["ret"]),
                                          P(out["path"]), P(out["count"]), P(out["steps"]), _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("kind", ["plain", "bank3-respawn", "f16", "stage_1", "orbit4-noise-gazebo", "bank3-noise-f16", "noise-f16", "per-env"])
def test_evaluate_hist_equals_the_stepping_loop(kind):
    quota = 3
    flat = _actor()[1]
    tabs = []
    for fn in (reference_table_hist, kernel_table_hist):
        s = make_sim(kind, seed=21)
        try:
            tabs.append(fn(s, flat, quota, quota * CAP))
        finally:
            s.close()
    want, got = tabs
    print(f"{kind}: outcomes {np.bincount(want['flags'].reshape(-1), minlength=5)[[1, 2, 4]]} steps {want['steps']}")
    assert (want["count"] == quota).all() and len(set(np.unique(want["flags"]).tolist())) >= 2
    for k in ("count", "steps", "flags", "length"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{kind}: {k}")
    for k in ("ret", "path"):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=f"{kind}: {k}")


@pytest.mark.parametrize("kind", ["plain", "bank3-noise-f16"])
def test_evaluate_hist_does_not_depend_on_the_placement(kind):
    """test_rollout_hist_does_not_depend_on_the_placement through navsim_evaluate_mlp64_hist: every env records its first three
    episodes whichever workgroup it plays in (`steps` is per workgroup and left out)"""
    quota = 3
    flat = _actor()[1]
    tabs = []
    for base, n in ((0, N),) + SHARDS:
        s = make_sim(kind, n, seed=21, env_id_base=base)
        try:
            tabs.append(kernel_table_hist(s, flat, quota, quota * CAP))
        finally:
            s.close()
    whole, parts = tabs[0], tabs[1:]
    assert (whole["count"] == quota).all() and len(set(np.unique(whole["flags"]).tolist())) >= 2
    for k in ("count", "flags", "length", "ret", "path"):
        got = np.concatenate([p[k] for p in parts], axis=-1)
        np.testing.assert_array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                                      whole[k].view(np.uint32) if got.dtype == np.float32 else whole[k], err_msg=f"{kind}: {k}")
    assert not np.array_equal(parts[1]["ret"], whole["ret"][:, :16])


def test_evaluate_hist_refuses_more_than_4096_envs():
    n, fill = 4097, 77
    s = make_sim("plain", n)
    try:
        obs0 = torch.empty((n, 16), device=DEV)
        s.reset(obs0)
        tab = [torch.full((1, n), fill, dtype=dt, device=DEV) for dt in (torch.uint8, torch.int32, torch.float32, torch.float32)]
        cnt = torch.full((n,), fill, dtype=torch.int32, device=DEV)
        stp = torch.full(((n + 15) // 16,), fill, dtype=torch.int32, device=DEV)
        rc = lib().navsim_evaluate_mlp64_hist(s._h, P(_actor()[1]), P(obs0), 1, CAP, *[P(x) for x in tab], P(cnt), P(stp), _st())
        assert rc == -1 and b"navsim_evaluate_mlp64_hist" in lib().navsim_last_error() and b"4096" in lib().navsim_last_error()
        torch.cuda.synchronize()
        for x in tab + [cnt, stp]:
            assert bool((x == fill).all())
    finally:
        s.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing():
    L = lib()
    flat = _actor()[1]
    # 36 beams
    s = NavSim(16, n_beams=36, max_episode_steps=CAP, auto_reset=True, device=DEV)
    s.set_map(maps.by_name("stage_1"))
    b = dict(obs=torch.zeros((3, 16, 42), device=DEV), act=torch.full((2, 16, 2), 7.0, device=DEV), logp=torch.zeros((2, 16), device=DEV),
             reward=torch.zeros((2, 16), device=DEV), flag=torch.zeros((2, 16), dtype=torch.uint8, device=DEV))
    var = torch.tensor(VAR, device=DEV)

    def roll(sim, prm, obs, act):
        return L.navsim_rollout_mlp64_hist(sim._h, P(prm), P(obs), P(act), P(b["logp"]), P(b["reward"]), P(b["flag"]), P(b["flag"]),
                                           P(b["flag"]), None, None, None, P(var), 1, None, 2, _st())

    assert roll(s, flat, b["obs"], b["act"]) == -1 and b"10" in L.navsim_last_error()
    cnt, stp = torch.zeros(16, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = [torch.zeros((1, 16), dtype=dt, device=DEV) for dt in (torch.uint8, torch.int32, torch.float32, torch.float32)]
    rc = L.navsim_evaluate_mlp64_hist(s._h, P(flat), P(b["obs"]), 1, 5, *[P(x) for x in tab], P(cnt), P(stp), _st())
    assert rc == -1 and b"navsim_evaluate_mlp64_hist" in L.navsim_last_error() and b"10" in L.navsim_last_error()
    s.close()
    # null and misaligned pointers
    s = make_sim("plain", 16)
    obs = torch.zeros((3, 16, 16), device=DEV)
    assert roll(s, None, obs, b["act"]) == -1
    assert roll(s, flat, None, b["act"]) == -1
    assert roll(s, flat.view(-1)[1:], obs, b["act"]) == -1 and b"aligned" in L.navsim_last_error()
    assert roll(s, flat, obs.view(-1)[1:], b["act"]) == -1 and b"aligned" in L.navsim_last_error()
    assert roll(s, flat, obs, b["act"].view(-1)[1:]) == -1 and b"aligned" in L.navsim_last_error()
    rc = L.navsim_evaluate_mlp64_hist(s._h, P(flat), P(obs.view(-1)[1:]), 1, 5, *[P(x) for x in tab], P(cnt), P(stp), _st())
    assert rc == -1 and b"aligned" in L.navsim_last_error()
    rc = L.navsim_evaluate_mlp64_hist(s._h, P(flat), None, 1, 5, *[P(x) for x in tab], P(cnt), P(stp), _st())
    assert rc == -1
    s.close()
    o = torch.zeros((2, 4, 16), device=DEV)
    e = torch.zeros((1, 4), dtype=torch.uint8, device=DEV)
    out = torch.full((2, 4, HIST_DIM), 7.0, device=DEV)
    for args in ((None, 0, P(e), 2, 4, P(out)), (P(o), 0, None, 2, 4, P(out)), (P(o), 0, P(e), 2, 4, None), (P(o), 0, P(e), 0, 4, P(out)),
                 (P(o), 0, P(e), 2, 0, P(out)), (P(o.view(-1)[1:]), 0, P(e), 2, 4, P(out)), (P(o), 0, P(e), 2, 4, P(out.view(-1)[1:]))):
        assert L.navsim_stack_rows(*args, _st()) == -1 and b"navsim_stack_rows" in L.navsim_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((b["act"] == 7.0).all())
    # the Python wrappers: a 16-column actor, a 36-beam env
    env = VecEnv(16, map="stage_1", max_episode_steps=CAP, device=DEV)
    a16 = nets.flat_actor_params(nets.make_policy("mlp64x2", 16)[0]).to(DEV)
    assert a16.numel() == 5378
    with pytest.raises(NavsimError, match="7042"):
        env.rollout_mlp64(a16, 4, VAR, history=True)
    with pytest.raises(NavsimError, match="7042"):
        env.evaluate_policy(a16, 1, history=True)
    with pytest.raises(ValueError, match="history"):
        env.evaluate_policy(a16, 1, policy="resmlp512", history=True)
    out = env.rollout_mlp64(flat, 4, VAR, history=True)
    assert out.obs.shape == (5, 16, 16) and out.act.shape == (4, 16, 2)
    env.close()
    env = VecEnv(16, map="stage_1", n_beams=36, max_episode_steps=CAP, device=DEV)
    with pytest.raises(NavsimError, match="10 beams"):
        env.rollout_mlp64(flat, 4, VAR, history=True)
    with pytest.raises(ValueError, match="history"):
        env.evaluate_policy(flat, 1, history=True)
    with pytest.raises(ValueError, match="n_beams == 10"):
        ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", scan_history=True, rollout_len=4))
    env.close()


# ---------------------------------------------------------------- 7. guarded allocations
@pytest.mark.parametrize("kind", ["plain", "f16", "bank3-respawn", "orbit4-noise-gazebo", "bank3-noise-f16"])
def test_rollout_hist_outputs_guarded(kind):
    """every argument of navsim_rollout_mlp64_hist inside a guarded allocation, at a 256-byte boundary and at the minimum alignment:
    guards intact, every row written, outputs identical between the placements and equal to the plain run's"""
    flat = _actor()[1]
    want, _ = _kernel_of(kind)

    def call(g):
        s = make_sim(kind)
        try:
            z = _buffers(s, T)
            b = dict(obs=g.out((T + 1, N, 16), s.obs_dtype, 16), act=g.out((T, N, 2), torch.float32, 8))
            for f in ("logp", "reward"):
                b[f] = g.out((T, N), torch.float32, 4)
            for f in ("done", "arrive", "ended"):
                b[f] = g.out((T, N), torch.uint8, 1)
            for f in ("ep_return", "ep_length", "ep_path"):   # written where an episode ends only: in-out, zeroed
                b[f] = g.io(z[f], 4)
            start(s, b["obs"][0])
            pr, var = g.inp(flat, 16), g.inp(torch.tensor([VAR], device=DEV), 4)
            base = g.inp(torch.tensor([STEP_BASE], dtype=torch.int32, device=DEV), 4)
            rc = lib().navsim_rollout_mlp64_hist(s._h, P(pr), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                                                 P(b["arrive"]), P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]),
                                                 P(var), ACT_SEED, P(base), T, _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            return {f: b[f].clone() for f in FIELDS}
        finally:
            s.close()

    got = run_both(DEV, call, f"navsim_rollout_mlp64_hist {kind}")
    for f in FIELDS:
        assert same(got[f], want[f]), f


@pytest.mark.parametrize("kind", ["plain", "f16", "bank3-respawn", "orbit4-noise-gazebo", "bank3-noise-f16"])
def test_evaluate_hist_outputs_guarded(kind):
    flat = _actor()[1]
    quota = 2

    def call(g):
        s = make_sim(kind, seed=21)
        try:
            obs0 = g.out((N, 16), s.obs_dtype, 16)
            s.reset(obs0)
            pr = g.inp(flat, 16)
            fl = g.out((quota, N), torch.uint8, 1)
            ln, rt, pa = g.out((quota, N), torch.int32, 4), g.out((quota, N), torch.float32, 4), g.out((quota, N), torch.float32, 4)
            cnt, stp = g.out((N,), torch.int32, 4), g.out(((N + 15) // 16,), torch.int32, 4)
            rc = lib().navsim_evaluate_mlp64_hist(s._h, P(pr), P(obs0), quota, quota * CAP, P(fl), P(ln), P(rt), P(pa), P(cnt), P(stp), _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            assert bool((cnt == quota).all())
            return fl
        finally:
            s.close()

    run_both(DEV, call, f"navsim_evaluate_mlp64_hist {kind}")


def test_single_env_drop_in_returns_the_history_row():
    """Env(scan_history=True) beside a plain Env on the same seed and actions: the 42-vector is stack_rows_reference of the plain
    env's rows under the flag the step wrote (the cuts of the host window are covered in tests/test_scan_history_cpu.py)"""
    from navbot_ppo_amd.env import Env
    hist, plain = Env(True, seed=3, movers="orbit4", scan_history=True), Env(True, seed=3, movers="orbit4")
    try:
        rows, got, flags = [plain.reset()], [hist.reset()], []
        rng = np.random.default_rng(2)
        past = np.zeros(2, np.float32)
        for _ in range(6):
            a = np.array([rng.uniform(0, 1), rng.uniform(-1, 1)], np.float32)
            o, r, d, ar = plain.step(a, past)
            o2, r2, d2, ar2 = hist.step(a, past)
            assert (r, d, ar) == (r2, d2, ar2)
            rows.append(o)
            got.append(o2)
            flags.append(d or ar)   # (an Env has no time-out: ended = done | arrive)
            past = a
    finally:
        hist.close()
        plain.close()
    want = stack_rows_reference(np.stack(rows)[:, None, :].astype(np.float32), np.array(flags, np.uint8)[:, None])[:, 0]
    assert got[0].shape == (HIST_DIM,) and got[0].dtype == np.float64
    assert np.array_equal(np.stack(got), want.astype(np.float64))
    assert not np.array_equal(want[3, 16:26], want[3, 26:36])   # the frames differ once the robot has moved


# ---------------------------------------------------------------- 8. the trainer
def test_trainer_with_scan_history(tmp_path):
    env = VecEnv(64, movers="random:4")
    cfg = ppo.PPOConfig(policy="mlp64x2", scan_history=True, rollout_len=32, n_updates_per_iteration=2, eval_every=1, eval_episodes=8,
                        output_dir=str(tmp_path), method_name="m")   # (the output directory: where the checkpoint below goes)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.uses_persistent_rollout and tr.updater.fused_mlp64 and tr.updater.obs_dim == HIST_DIM
    assert tr.obs_buf.shape == (33, 64, 16) and tr.hist_buf.shape == (33, 64, HIST_DIM)
    assert sum(p.numel() for p in tr.actor.parameters()) == 7042
    before = tr.updater.fp.flat.clone()
    for _ in range(2):
        lg = tr.iteration()
        assert all(math.isfinite(lg[k]) for k in ("actor_loss", "critic_loss", "approx_kl")), lg
        assert "eval_success" in lg and lg["eval_episodes"] == 8
    torch.cuda.synchronize()
    assert not torch.equal(before, tr.updater.fp.flat)
    print(f"episode ends in the last rollout: {int(tr.ended_buf.sum())}")
    want = stack_rows_reference(tr.obs_buf.cpu().numpy(), tr.ended_buf.cpu().numpy())
    assert same(tr.hist_buf.cpu(), torch.from_numpy(want))
    pa, _ = tr.save_checkpoint()
    tr._eval_env.close()
    env.close()
    actor, pol = ev.load_actor(pa, DEV)
    assert pol == "mlp64x2" and ev.reads_scan_history(actor)
    kw = dict(num_episodes=8, n_parallel=8, seed=4, log=None, movers="random:4")
    sp = ev.evaluate(actor, persistent=True, **kw)
    sl = ev.evaluate(actor, **kw)
    assert sp["episodes"] == sl["episodes"] == 8
    assert [r[1:5] for r in sp["rows"]] == [r[1:5] for r in sl["rows"]]     # success, collision, timeout, length
    np.testing.assert_allclose([r[5] for r in sp["rows"]], [r[5] for r in sl["rows"]], rtol=1e-4, atol=1e-3)


UPDATE_CASES = {   # name -> (PPOConfig options, VecEnv options)
    "defaults": ({}, {}),                                  # bf16x3 on the prepared pieces of the batch
    "f32": (dict(update_arith="f32"), {}),
    "minibatch": (dict(minibatch_size=96, minibatch_shuffle="epoch", max_grad_norm=0.5), {}),
    "f16-returns": (dict(bootstrap_truncated=True, gae_lambda=0.95, norm_reward=True), dict(obs_f16=True)),
    "adaptive-lr": (dict(lr_schedule="adaptive"), {}),
    "target-kl": (dict(target_kl=0.01), {}),
}


@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_the_update_reads_the_rows_the_rule_prescribes(case):
    """Two trainers built alike.  A runs iteration() twice.  B runs it once, then rollout() -- the same buffers as A's second
    rollout, bit for bit -- and then the update as iteration() calls it, but on a freshly allocated tensor holding
    stack_rows_reference of its obs_buf / ended_buf.  The fused paths are deterministic, so parameters and Adam's moments come out
    bit-identical if and only if A's second update consumed exactly those rows -- not the first iteration's, which lie behind the
    same pointer, shape and version counter (hist_buf[:T] is a view of a buffer the kernels rewrite every iteration)."""
    cfg_kw, env_kw = UPDATE_CASES[case]
    n, t_len = 64, 32
    trainers = []
    for _ in range(2):
        env = VecEnv(n, map="stage_1", max_episode_steps=20, seed=1, movers="random:4", **env_kw)
        cfg = ppo.PPOConfig(policy="mlp64x2", scan_history=True, rollout_len=t_len, max_episode_steps=20, n_updates_per_iteration=3, seed=2,
                            **cfg_kw)
        trainers.append(ppo.PPOTrainer(env, cfg))
    A, B = trainers
    names = ("obs_buf", "act_buf", "logp_buf", "ended_buf", "rtg_buf")
    try:
        assert A.scan_history and A.updater.obs_dim == HIST_DIM and same(A.updater.fp.flat, B.updater.fp.flat)
        A.iteration()
        snap = {}
        rollout = A.rollout

        def recording_rollout():
            rollout()
            snap.update({k: getattr(A, k).clone() for k in names})
            snap["flat"] = A.updater.fp.flat.clone()

        A.rollout = recording_rollout
        A.iteration()
        B.iteration()
        B.rollout()
        torch.cuda.synchronize()
        for k in names:
            assert same(getattr(B, k), snap[k]), f"{case}: {k} of the second rollout"
        assert same(B.updater.fp.flat, snap["flat"])
        n_ends = int(B.ended_buf.sum())
        print(f"{case}: episode ends in the second rollout: {n_ends}")
        assert n_ends >= n   # the cuts matter: rows that start an episode all over the batch
        rows = torch.from_numpy(stack_rows_reference(B.obs_buf.cpu().numpy(), B.ended_buf.cpu().numpy()))[:t_len]
        rows = rows.reshape(t_len * n, HIST_DIM).to(DEV)
        assert rows.data_ptr() != B.hist_buf.data_ptr() and rows.dtype == B.hist_buf.dtype
        B.updater.update(rows, B.act_buf.reshape(t_len * n, 2), B.logp_buf.reshape(t_len * n), B.rtg_buf.reshape(t_len * n), B.var_host,
                         **({} if B._gae is None else dict(adv_raw=B._gae[0], V0=B._gae[1])))
        torch.cuda.synchronize()
        assert (B._gae is not None) == (case == "f16-returns")
        assert not same(A.updater.fp.flat, snap["flat"])   # the update moved the parameters
        assert same(A.updater.fp.flat, B.updater.fp.flat), f"{case}: parameters"
        assert same(A.updater._adam_m, B.updater._adam_m), f"{case}: Adam's first moment"
        assert same(A.updater._adam_v, B.updater._adam_v), f"{case}: Adam's second moment"
        assert A.updater._adam_t == B.updater._adam_t > 0
    finally:
        A.env.close()
        B.env.close()
