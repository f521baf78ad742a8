"""A bank of tapes, one scenario per env (navsim_set_mover_bank): the tape is chosen where it is read -- per env, inside every
stepping kernel, the reset / spawn-scan kernel and navsim_raycast -- and a tape may bring goal rectangles of its own.

The common setup: 40 envs (two full 16-env workgroups and a ragged one), three blade tapes (P, M, radius) = (5, 3, 0.75),
(8, 17, 0.60), (13, 32, 0.90) banked to Pmax = 13, Mmax = 32, tape ids from default_rng(7) (10 / 13 / 17 envs per tape, at least two
tapes in every workgroup), per-tape phases as test_gpu_movers._phase0 draws them.  Every check has an exact reference that already
exists: the composed-map oracle of tests/_movers.py per tape, and a handle with navsim_set_movers on the un-padded tape."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _guards import Guards
from _movers import MoverOracle, blade_tape, tripwire_rows
from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, NavsimError, VecEnv
from test_gpu_parity import _actions

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, T, CAP = 40, 60, 25
TE = 40          # steps of the entry-point comparisons
SPECS = [(5, 3, 0.75), (8, 17, 0.60), (13, 32, 0.90)]
K = len(SPECS)
R_NEAR = 0.45   # the persistent forms cap an episode at 9 steps: their blades turn 0.45 m from the spawn pose (test_gpu_movers.R_NEAR)
TID = np.random.default_rng(7).integers(0, K, N).astype(np.int32)
OBS_ATOL = 1e-6


def _phase0(P, M, n):   # (test_gpu_movers._phase0)
    return np.random.default_rng(1000 * P + M).integers(0, P, n).astype(np.int32)


def _tapes(radius=None):
    return [blade_tape(P, M, radius=r if radius is None else radius) for P, M, r in SPECS]


PH_OF_TAPE = [_phase0(P, M, N) for P, M, _ in SPECS]          # tape k's phases for all 40 envs (a single-tape handle's)
PH0 = np.array([PH_OF_TAPE[TID[i]][i] for i in range(N)], np.int32)   # ... and the bank's: each env that of its own tape
COLS = [np.flatnonzero(TID == k) for k in range(K)]


def test_the_setup_is_what_the_cases_assume():
    assert [len(c) for c in COLS] == [10, 13, 17]
    for w in range(3):
        assert len(set(TID[16 * w:16 * w + 16].tolist())) >= 2
    bank, periods, _ = maps.mover_bank(_tapes())
    assert bank.shape == (3, 13, 32, 4) and periods.tolist() == [5, 8, 13]


def bits(x):
    """float tensors as bit patterns (a NaN compares equal to itself)"""
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def _static(n=N, rects=None, **kw):
    """a stage_1 handle with stage_1's goal rectangles (+ `rects` appended to both `which`), no movers yet"""
    g = NavSim(n, device=DEV, **kw)
    rr, rs = maps.goal_rects("stage_1")
    if rects is not None:
        rr, rs = np.concatenate([rr, rects]), np.concatenate([rs, rects])
    g.set_goal_rects(0, rr)
    g.set_goal_rects(1, rs)
    g.set_map(maps.stage_1())
    return g


def _banked(radius=None, rects=None, bank=None, tid=TID, ph0=PH0, **kw):
    g = _static(**kw)
    b, periods, _ = maps.mover_bank(_tapes(radius))
    g.set_mover_bank(b if bank is None else bank, periods, tid, ph0, rects)
    return g


def _single(k, radius=None, rects=None, **kw):
    """the handle tape k's columns are compared with: navsim_set_movers on the un-padded tape, tape k's phases for every env"""
    g = _static(rects=rects, **kw)
    g.set_movers(_tapes(radius)[k], PH_OF_TAPE[k])
    return g


# ---------------------------------------------------------------- 1. lock step against the oracle, one MoverOracle per tape
@functools.lru_cache(maxsize=None)
def _lock_actions():
    return _actions(np.random.default_rng(31), T, N)


def _record_steps(g, acts):
    """reset + one navsim_step per row of acts: every output of every step, and the state at the end, on the host"""
    io = g.alloc_io()
    rows = [dict(obs=g.reset(io.obs).float().cpu().numpy())]
    for a in acts:
        g.step(torch.from_numpy(a).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended, io.ep_return, io.ep_length, ep_path=io.ep_path)
        rows.append({k: getattr(io, k).float().cpu().numpy() if k == "obs" else getattr(io, k).cpu().numpy()
                     for k in ("obs", "reward", "done", "arrive", "ended", "ep_return", "ep_length", "ep_path")})
    return rows, g.get_state()


def test_lockstep_against_one_oracle_per_tape():
    acts = _lock_actions()
    g = _banked(max_episode_steps=CAP, auto_reset=True, seed=5)
    inf = g.info()
    assert (inf["step_epb"], inf["step_waves"]) == (16, 8), inf
    assert g.movers_tapes == K and g.movers_period == 13 and g.movers_segments == 32
    rows, state = _record_steps(g, acts)
    g.close()
    s = _static(max_episode_steps=CAP, auto_reset=True, seed=5)
    static_done = sum(int(r["done"].sum()) for r in _record_steps(s, acts)[0][1:])
    s.close()
    rr, rs = maps.goal_rects("stage_1")
    for k, tape in enumerate(_tapes()):
        c = COLS[k]
        cpu = MoverOracle(N, maps.stage_1(), tape, PH_OF_TAPE[k], watch=False, max_episode_steps=CAP, seed=5)
        cpu.set_goal_rects(0, rr)
        cpu.set_goal_rects(1, rs)
        np.testing.assert_allclose(rows[0]["obs"][c], cpu.reset()[c], rtol=0, atol=OBS_ATOL)
        done = exact = total = 0
        in_scan = np.ones(len(c), bool)
        for t in range(T):
            out, got = cpu.step(acts[t]), rows[t + 1]
            for f in ("done", "arrive", "ended"):
                np.testing.assert_array_equal(got[f][c], out[f][c], err_msg=f"tape {k} {f}, step {t}")
            np.testing.assert_allclose(got["obs"][c], out["obs"][c], rtol=0, atol=OBS_ATOL, err_msg=f"tape {k} obs, step {t}")
            np.testing.assert_allclose(got["reward"][c], out["reward"][c], rtol=1e-5, atol=1e-5, err_msg=f"tape {k} reward, step {t}")
            e = out["ended"].astype(bool)[c]
            np.testing.assert_array_equal(got["ep_length"][c][e], out["ep_length"][c][e])
            done += int(out["done"][c].sum())
            exact += int((got["obs"][c] == out["obs"][c]).all(axis=1).sum())
            total += len(c)
            in_scan &= cpu.tape_in_scan()[c]
        sc = cpu.get_state()
        np.testing.assert_allclose(state["pose"][c], sc["pose"][c], rtol=0, atol=1e-11)
        for f in ("goal", "ep_step", "rng_ctr"):
            np.testing.assert_array_equal(state[f][c], sc[f][c])
        print(f"tape {k}: done {done} (static map {static_done}) exact rows {exact}/{total} tape in every scan {in_scan.all()}")
        assert exact > 0.99 * total
        assert in_scan.all()     # every row of every env has a tape segment in its scan
        assert done >= 10        # the tape ends episodes ...
    assert static_done == 0      # ... that the static map alone does not


# ---------------------------------------------------------------- 2. bit identity against single-tape handles
def _entry_points(make, **kw):
    """The reset observation, navsim_step, navsim_raycast and navsim_step_seq on the handles make(**options) builds:
    {name: [(tensor, its env axis)]}"""
    out = {}
    acts = torch.from_numpy(_actions(np.random.default_rng(45), TE, N)).to(DEV)
    # reset observation + navsim_step (auto-reset, cap 25, 40 steps: collisions with the blades, time-outs and phase wraps inside the run)
    g = make(max_episode_steps=CAP, auto_reset=True, seed=8, **kw)
    io = g.alloc_io()
    rec = [(g.reset(io.obs).clone(), 0)]
    for t in range(TE):
        g.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
        rec += [(getattr(io, f).clone(), 0) for f in ("obs", "reward", "done", "arrive", "ended")]
    out["reset+step"] = rec
    # navsim_raycast after set_state(ep_step=...)
    rng = np.random.default_rng(44)
    g.set_state(ep_step=rng.integers(0, 50, N).astype(np.int32))
    pose = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(-7, 7, N)], 1)
    out["raycast"] = [(g.raycast(torch.from_numpy(pose)).clone(), 0)]
    g.close()
    # navsim_step_seq
    g = make(max_episode_steps=CAP, auto_reset=True, seed=8, **kw)
    z = lambda dt=torch.float32, *s: torch.zeros((TE, N) + s, dtype=dt, device=DEV)
    seq = [z(g.obs_dtype, 16), z(), z(torch.uint8), z(torch.uint8), z(torch.uint8)]
    o0 = torch.empty((N, 16), dtype=g.obs_dtype, device=DEV)
    g.reset(o0)
    g.step_seq(acts, *seq)
    out["step_seq"] = [(x, 1) for x in seq]
    g.close()
    return out


def _rollouts(make_env_movers, radius, **kw):
    """both persistent rollouts (16 steps, episodes capped at 9) and both evaluation tables, through the trainer / VecEnv"""
    from test_gpu_evaluate import _actor
    out = {}
    for policy in ("mlp64x2", "resmlp512"):
        env = VecEnv(N, map="stage_1", max_episode_steps=9, seed=3, **kw)
        make_env_movers(env.sim, radius)
        cfg = ppo.PPOConfig(rollout_len=16, max_episode_steps=9, n_updates_per_iteration=1, policy=policy, seed=5,
                            persistent_rollout=True, use_graph=False)
        tr = ppo.PPOTrainer(env, cfg)
        assert tr.uses_persistent_rollout
        tr.rollout()
        torch.cuda.synchronize()
        ended = tr.ended_buf.bool()
        out["rollout_" + policy] = ([(b.clone(), 1) for b in (tr.obs_buf, tr.act_buf, tr.logp_buf, tr.rew_buf, tr.done_buf, tr.arrive_buf,
                                                               tr.ended_buf)] +
                                    [(torch.where(ended, b, torch.zeros_like(b)), 1) for b in (tr.epret_buf, tr.eplen_buf, tr.eppath_buf)])
        assert int(tr.ended_buf.sum()) >= N
        tab = env.evaluate_policy(_actor(policy, 16)[1], 2, policy=policy)
        torch.cuda.synchronize()
        assert int(tab.count.min()) >= 2
        out["evaluate_" + policy] = [(x.clone(), 1) for x in (tab.flags, tab.length, tab.ret, tab.path)]
        env.close()
    return out


def _assert_columns_equal(bank_out, single_out, k, what):
    idx = torch.from_numpy(COLS[k]).to(DEV)
    for name in bank_out:
        assert len(bank_out[name]) == len(single_out[name])
        for j, ((x, ax), (y, _)) in enumerate(zip(bank_out[name], single_out[name])):
            assert torch.equal(bits(x.index_select(ax, idx)), bits(y.index_select(ax, idx))), f"{what}: {name} #{j}, tape {k}"


SENSOR = [pytest.param({}, id="plain"), pytest.param(dict(lidar_noise_sigma=0.02, lidar_below_min="gazebo"), id="noise-gazebo"),
          pytest.param(dict(obs_f16=True), id="f16")]


@pytest.mark.parametrize("kw", SENSOR)
def test_step_entry_points_bit_identical_to_single_tape_handles(kw):
    """The single-tape handles hold the un-padded tapes: their M (3, 17, 32) and mov_pack_log2 differ from the bank's."""
    got = _entry_points(lambda **o: _banked(**o), **kw)
    assert int(sum(int(x.sum()) for (x, _) in got["reset+step"][3::5])) > 0   # the tapes end episodes in this run
    for k in range(K):
        _assert_columns_equal(got, _entry_points(lambda **o: _single(k, **o), **kw), k, "steps")


@pytest.mark.parametrize("kw", SENSOR)
def test_rollouts_and_evaluations_bit_identical_to_single_tape_handles(kw):
    def bank_movers(sim, radius):
        b, periods, _ = maps.mover_bank(_tapes(radius))
        sim.set_mover_bank(b, periods, TID, PH0)
    got = _rollouts(bank_movers, R_NEAR, **kw)
    assert int(got["rollout_mlp64x2"][4][0].sum()) > 0   # collisions with the blades inside the launch
    for k in range(K):
        want = _rollouts(lambda sim, radius: sim.set_movers(_tapes(radius)[k], PH_OF_TAPE[k]), R_NEAR, **kw)
        _assert_columns_equal(got, want, k, "persistent")


# ---------------------------------------------------------------- 3. tripwire on the padding
def _tripwire_bank(radius=None):
    """(the plain NaN-padded bank, a [K * Pmax + 2, M, 4] tensor whose rows 1 .. K * Pmax are the bank with tripwire_rows -- a wall
    0.3 m round the spawn pose -- in the row in front of tape 0, the row behind tape K-1 and rows period[k] .. Pmax-1 of every tape)"""
    bank, periods, _ = maps.mover_bank(_tapes(radius))
    Kb, Pmax, M, _ = bank.shape
    wire = tripwire_rows(M)
    trap = bank.copy()
    for k in range(Kb):
        trap[k, periods[k]:] = wire
    big = np.concatenate([wire[None], trap.reshape(Kb * Pmax, M, 4), wire[None]])
    return bank, torch.from_numpy(np.ascontiguousarray(big)).to(DEV)


def _tripwire_phases():
    ph = PH0.copy()
    for k, (P, _, _) in enumerate(SPECS):   # both ends of every tape's range occur
        ph[COLS[k][0]], ph[COLS[k][1]] = 0, P - 1
    return ph


@pytest.mark.parametrize("radius", [pytest.param(None, id="steps"), pytest.param(R_NEAR, id="rollouts")])
def test_rows_outside_a_tape_are_never_read(radius):
    """A kernel that takes Pmax for a tape's period, or steps across a tape boundary, casts a wall 0.3 m from the spawn pose that the
    plain bank does not hold: its scans change."""
    plain, big = _tripwire_bank(radius)
    ph = _tripwire_phases()
    inner = big[1:-1].view(K, 13, 32, 4)
    assert inner.data_ptr() % 16 == 0 and inner.data_ptr() == big.data_ptr() + 32 * 16
    outs = []
    for bank in (plain, inner):
        if radius is None:
            o = _entry_points(lambda **kw: _banked(bank=bank, ph0=ph, **kw))
        else:
            o = _rollouts(lambda sim, r: sim.set_mover_bank(bank, [5, 8, 13], TID, ph), radius)
        outs.append(o)
    for name in outs[0]:
        for j, ((x, _), (y, _)) in enumerate(zip(*[o[name] for o in outs])):
            assert torch.equal(bits(x), bits(y)), f"{name} #{j}"
    # the wire itself is seen where it is a tape's row: a bank whose tape 0 has its period raised to Pmax casts it
    g = _static(seed=8)
    g.reset(g.alloc_io().obs)
    g.set_state(ep_step=np.full(N, 6, np.int32))   # tape 0, phase0 in [0, 5): rows 6 .. 10 under period 13 (the wire), 1 .. 4, 0 under 5
    g.set_mover_bank(inner, [13, 8, 13], TID, ph)
    seen = g.raycast(torch.zeros((N, 3), dtype=torch.float64)).cpu().numpy()
    g.set_mover_bank(inner, [5, 8, 13], TID, ph)
    clear = g.raycast(torch.zeros((N, 3), dtype=torch.float64)).cpu().numpy()
    g.close()
    # (the wire's far corner is hypot(0.332, 0.3) = 0.447 m from the sensor; a blade ring leaves some beam a longer way)
    assert (seen[COLS[0]].max(axis=1) < 0.46).all() and (clear[COLS[0]].max(axis=1) > 0.46).all()
    np.testing.assert_array_equal(seen[COLS[1]], clear[COLS[1]])


# ---------------------------------------------------------------- 4. goal rectangles per tape
QUADS = np.array([[[0.0, 9.0, 0.0, 9.0]], [[-9.0, 0.0, 0.0, 9.0]], [[-9.0, 0.0, -9.0, 0.0]]])   # tape k's one rectangle


def _goal_run(g):
    """reset + 60 lock-step actions with auto-reset and the arrival re-spawn: per step outputs and the goal of every env"""
    io = g.alloc_io()
    rec, goals = [g.reset(io.obs).clone()], [g.get_state()["goal"].copy()]
    for a in _lock_actions():
        g.step(torch.from_numpy(a).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
        rec += [getattr(io, f).clone() for f in ("obs", "reward", "done", "arrive", "ended")]
        goals.append(g.get_state()["goal"].copy())
    g.close()
    return rec, np.stack(goals)   # [T + 1, N, 2]


@pytest.mark.parametrize("respawn", [False, True], ids=["reset-draw", "respawn-draw"])
def test_goal_rectangles_of_the_env_tape(respawn):
    """respawn-draw: with the arrival re-spawn on, the rectangles also reject its draw (`which` = 1); the counts below are those of
    the common setup (reset draws only)."""
    kw = dict(max_episode_steps=CAP, auto_reset=True, seed=5, respawn_on_arrive=respawn)
    rec, goals = _goal_run(_banked(rects=QUADS, **kw))
    _, goals_free = _goal_run(_banked(**kw))
    for k in range(K):
        c = COLS[k]
        want, goals_k = _goal_run(_single(k, rects=QUADS[k], **kw))   # the quadrant among the HANDLE's rectangles, both `which` (4 + 1 of 16)
        idx = torch.from_numpy(c).to(DEV)
        for j, (x, y) in enumerate(zip(rec, want)):
            assert torch.equal(bits(x.index_select(0, idx)), bits(y.index_select(0, idx))), f"tape {k} #{j}"
        np.testing.assert_array_equal(goals[:, c], goals_k[:, c])
        q = QUADS[k, 0]
        gx, gy = goals[:, c, 0], goals[:, c, 1]
        assert not ((q[0] <= gx) & (gx <= q[1]) & (q[2] <= gy) & (gy <= q[3])).any()   # no goal of these envs in their quadrant
        changed = int((goals[:, c] != goals_free[:, c]).any(axis=(0, 2)).sum())
        print(f"tape {k}: the quadrant changes the goal sequence of {changed} of {len(c)} envs")
        assert respawn or changed >= 5


def test_goal_rectangles_do_not_apply_to_goal_tables():
    st, gl, dmin, dmax = maps.spawn_tables("stage1")
    st, gl = maps.open_tables(maps.stage_1(), st, gl)
    outs = []
    for rects in (None, QUADS):
        g = _static(max_episode_steps=CAP, auto_reset=True, seed=5)
        g.set_spawn_sampler(st, gl, dmin, dmax)
        b, periods, _ = maps.mover_bank(_tapes())
        g.set_mover_bank(b, periods, TID, PH0, rects)
        outs.append(_goal_run(g))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert torch.equal(bits(x), bits(y))
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------- 5. shards
def test_two_shards_reproduce_one_handle():
    """assign="random", phase="random": ids and phases come from (map_seed, global env id) only -- per step and in one persistent
    rollout, with sensor noise"""
    from test_gpu_evaluate import _actor
    b, periods, _ = maps.mover_bank(_tapes(R_NEAR))
    movers = dict(bank=b, periods=periods, assign="random", phase="random")
    kw = dict(map="stage_1", max_episode_steps=9, seed=3, map_seed=5, lidar_noise_sigma=0.02, movers=movers)
    flat = _actor("mlp64x2", 16)[1]
    acts = torch.from_numpy(_actions(np.random.default_rng(45), 24, N)).to(DEV)

    def run(n, base):
        env = VecEnv(n, env_id_base=base, **kw)
        rec = [env.reset().clone()]
        for t in range(24):
            env.step(acts[t, base:base + n])
            rec += [getattr(env.io, f).clone() for f in ("obs", "reward", "done", "ended")]
        env.reset()
        r = env.rollout_mlp64(flat, 16, 0.3, seed=11)
        rec += [x.transpose(0, 1).contiguous() for x in (r.obs[1:], r.act, r.logp, r.reward, r.done, r.ended)]   # env-major
        ids = env.sim.movers_tape_id.cpu().numpy()
        env.close()
        return rec, ids
    whole, ids = run(N, 0)
    lo, ids_lo = run(24, 0)
    hi, ids_hi = run(16, 24)
    assert len(set(ids.tolist())) == K
    np.testing.assert_array_equal(ids, np.concatenate([ids_lo, ids_hi]))
    for j, (w, a, c) in enumerate(zip(whole, lo, hi)):
        assert torch.equal(bits(w), bits(torch.cat([a, c]))), j
    assert sum(int(x.sum()) for x in whole[3:97:4]) > 0   # the blades end episodes in the per-step part


# ---------------------------------------------------------------- 6. contracts
def _short_run(g, n=N, steps=20):
    acts = torch.from_numpy(_actions(np.random.default_rng(43), steps, n)).to(DEV)
    io = g.alloc_io()
    rec = [g.reset(io.obs).clone()]
    for t in range(steps):
        g.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
        rec += [getattr(io, f).clone() for f in ("obs", "reward", "done", "ended")]
    return rec


def _same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_a_bank_of_one_tape_is_set_movers_and_each_call_replaces_the_other():
    kw = dict(max_episode_steps=9, auto_reset=True, seed=4)
    tape = _tapes()[2]
    b, periods, _ = maps.mover_bank(_tapes())

    def run(*calls):
        g = _static(**kw)
        for c in calls:
            c(g)
        rec, inf = _short_run(g), g.info()
        g.close()
        return rec, inf, (g.movers_tapes, g.movers_tape_id is None, g.movers_period)
    single = lambda g: g.set_movers(tape, PH_OF_TAPE[2])
    bank1 = lambda g: g.set_mover_bank(tape[None], None, None, PH_OF_TAPE[2])   # K = 1, no ids, no rectangles
    bank3 = lambda g: g.set_mover_bank(b, periods, TID, PH0, QUADS)
    off = lambda g: g.set_mover_bank(None)
    want1, want3, want0 = run(single), run(bank3), run()
    assert not _same(want1[0], want3[0]) and not _same(want1[0], want0[0])
    assert _same(run(bank1)[0], want1[0])                   # a K = 1 bank without rectangles gives the bits of set_movers
    got = run(bank3, single)                                # set_movers behind a bank replaces it, rectangles included
    assert _same(got[0], want1[0]) and got[2] == (1, True, 13)
    got = run(single, bank3)                                # ... and the other way round
    assert _same(got[0], want3[0]) and got[2] == (3, False, 13)
    got = run(bank3, off)                                   # off: the static handle and its kernels
    assert _same(got[0], want0[0]) and got[1] == want0[1] and got[2] == (0, True, 0)


def test_a_period_one_tape_is_per_env_clutter():
    """two clutter layouts and a moving tape in one batch: the period-1 envs see their pillars at every step, as a static map that
    holds them does"""
    centres = [[(0.9, 0.05), (0.9, -0.9)], [(0.9, -0.05), (0.3, 1.1)]]   # one pillar of each layout stands straight ahead of the spawn pose
    tapes = [maps.clutter_tape(c) for c in centres] + [_tapes()[1]]
    bank, periods, rects = maps.mover_bank(tapes, [maps.clutter_rects(c) for c in centres] + [[]])
    assert periods.tolist() == [1, 1, 8]
    ph = np.where(TID == 2, PH_OF_TAPE[1], 0).astype(np.int32)
    kw = dict(max_episode_steps=CAP, auto_reset=True, seed=5)
    g = _static(**kw)
    g.set_mover_bank(bank, periods, TID, ph, rects)
    got = _short_run(g, steps=40)
    g.close()
    for k in (0, 1):
        s = NavSim(N, device=DEV, **kw)
        rr, rs = maps.goal_rects("stage_1")
        s.set_goal_rects(0, np.concatenate([rr, maps.clutter_rects(centres[k])]))
        s.set_goal_rects(1, np.concatenate([rs, maps.clutter_rects(centres[k])]))
        s.set_map(np.concatenate([maps.stage_1(), tapes[k][0]]))   # the pillars as part of the static map
        want = _short_run(s, steps=40)
        s.close()
        idx = torch.from_numpy(COLS[k]).to(DEV)
        for j, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(bits(x.index_select(0, idx)), bits(y.index_select(0, idx))), (k, j)
    assert sum(int(x.index_select(0, torch.from_numpy(np.concatenate(COLS[:2])).to(DEV)).sum()) for x in got[3::4]) > 0   # pillars are hit


def _rc(fn, *a):
    return fn(*a), lib().navsim_last_error().decode()


def test_refusals_leave_the_previous_movers_in_force():
    L = lib()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    I = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.c_void_p)
    D = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    b, periods, _ = maps.mover_bank(_tapes())
    bank = torch.from_numpy(b).to(DEV)
    tid, ph = torch.from_numpy(TID).to(DEV), torch.from_numpy(PH0).to(DEV)
    per = I(periods)
    call = lambda h, *a: _rc(L.navsim_set_mover_bank, h, *a)
    g = NavSim(N, device=DEV, max_episode_steps=9, auto_reset=True, seed=4)
    assert call(g._h, P(bank), 3, 13, 32, per, P(tid), P(ph), None, 0, None)[0] == -3           # before set_map
    g.close()
    g = _single(2, max_episode_steps=9, auto_reset=True, seed=4)
    bad_tid, bad_ph = tid.clone(), ph.clone()
    bad_tid[17] = 3
    bad_ph[int(COLS[0][0])] = 5                                                                  # = the period of that env's tape
    neg_ph = ph.clone()
    neg_ph[3] = -1
    odd = torch.zeros(3 * 13 * 32 * 4 + 4, device=DEV)[1:]                                        # 4-byte aligned only
    cases = [((P(bank), 0, 13, 32, per, P(tid), P(ph), None, 0, None), "n_tapes"),
             ((P(bank), 3, 0, 32, per, P(tid), P(ph), None, 0, None), "max_period"),
             ((P(bank), 3, 65537, 32, per, P(tid), P(ph), None, 0, None), "max_period"),
             ((P(bank), 257, 65536, 32, per, None, None, None, 0, None), "2^24"),
             ((P(bank), 3, 13, 65, per, P(tid), P(ph), None, 0, None), "n_segments"),
             ((P(bank), 3, 13, 0, per, P(tid), P(ph), None, 0, None), "n_segments"),
             ((P(odd), 3, 13, 32, per, P(tid), P(ph), None, 0, None), "aligned"),
             ((P(bank), 3, 13, 32, None, P(tid), P(ph), None, 0, None), "periods"),
             ((P(bank), 3, 13, 32, I([5, 14, 13]), P(tid), P(ph), None, 0, None), "period"),
             ((P(bank), 3, 13, 32, I([5, 0, 13]), P(tid), P(ph), None, 0, None), "period"),
             ((P(bank), 3, 13, 32, per, P(bad_tid), P(ph), None, 0, None), "tape id"),
             ((P(bank), 3, 13, 32, per, P(tid), P(bad_ph), None, 0, None), "phase0"),
             ((P(bank), 3, 13, 32, per, P(tid), P(neg_ph), None, 0, None), "phase0"),
             ((P(bank), 3, 13, 32, per, P(tid), P(ph), D(np.zeros((3, 9, 4))), 9, None), "n_rects"),
             ((P(bank), 3, 13, 32, per, P(tid), P(ph), None, -1, None), "n_rects"),
             ((P(bank), 3, 13, 32, per, P(tid), P(ph), None, 2, None), "rectangles")]
    for args, word in cases:
        rc, msg = call(g._h, *args)
        assert rc == -1 and "navsim_set_mover_bank" in msg and word in msg, (word, rc, msg)
    with pytest.raises(NavsimError):   # the Python layer checks the tensors before a pointer crosses the ABI
        g.set_mover_bank(torch.zeros((3, 13, 32, 3)))
    with pytest.raises(NavsimError):
        g.set_mover_bank(bank, periods, np.zeros(N - 1, np.int32))
    with pytest.raises(NavsimError):
        g.set_mover_bank(bank, periods, TID, np.zeros(N, np.float32))
    with pytest.raises(NavsimError):
        g.set_mover_bank(bank, [5, 8])
    with pytest.raises(NavsimError):
        g.set_mover_bank(bank, periods, TID, PH0, np.zeros((3, 9, 4)))
    fresh = _single(2, max_episode_steps=9, auto_reset=True, seed=4)
    assert g.movers_tapes == 1 and _same(_short_run(g), _short_run(fresh))     # every refused call left tape 2 in force
    g.close()
    fresh.close()

    g36 = NavSim(32, n_beams=36, device=DEV)
    g36.set_map(maps.stage_1())
    rc, msg = call(g36._h, P(bank), 3, 13, 32, per, None, None, None, 0, None)
    assert rc == -1 and "36 beams" in msg and "not built" in msg
    g36.close()
    gp = NavSim(32, device=DEV)
    gp.set_map(maps.replicate_per_env(maps.stage_1(), 32), per_env=True)
    rc, msg = call(gp._h, P(bank), 3, 13, 32, per, None, None, None, 0, None)
    assert rc == -1 and "per-env static map" in msg and "not built" in msg
    gp.set_map(maps.stage_1())
    gp.set_mover_bank(bank, periods)
    with pytest.raises(NavsimError, match="not built"):
        gp.set_map(maps.replicate_per_env(maps.stage_1(), 32), per_env=True)
    gp.close()


def test_guarded_bank_ids_and_phases():
    """the bank at its 16-byte minimum alignment, ids and phases at 4 bytes, poisoned guards round all three: the same bits as at
    256-byte placements, through the C ABI"""
    L = lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    b, periods, _ = maps.mover_bank(_tapes())
    per = np.ascontiguousarray(periods, np.int32)
    runs = []
    for minimal in (False, True):
        gd = Guards(DEV, minimal)
        bank = gd.inp(torch.from_numpy(b), 16)
        tid = gd.inp(torch.from_numpy(TID), 4)
        ph = gd.inp(torch.from_numpy(PH0), 4)
        g = _static(max_episode_steps=9, auto_reset=True, seed=4)
        rc = L.navsim_set_mover_bank(g._h, P(bank), K, 13, 32, per.ctypes.data_as(C.c_void_p), P(tid), P(ph), None, 0, None)
        assert rc == 0, L.navsim_last_error().decode()
        rec = _short_run(g)
        rec.append(g.raycast(torch.zeros((N, 3), dtype=torch.float64)).clone())
        gd.check(f"navsim_set_mover_bank ({'minimum alignment' if minimal else '256-byte'} placement)")
        g.close()
        assert all(torch.isfinite(x.float()).all() for x in rec[:-1])   # a read of a poisoned guard would be a NaN
        runs.append(rec)
    assert _same(*runs)
    h = _banked(max_episode_steps=9, auto_reset=True, seed=4)
    assert _same(_short_run(h), runs[0][:-1])
    h.close()


# ---------------------------------------------------------------- 7. VecEnv / trainer
def test_vecenv_and_trainer_with_a_held_out_bank(tmp_path):
    env = VecEnv(32, map="stage_1", max_episode_steps=30, seed=3, movers="random:4")
    assert env.sim.movers_tapes == 4 and env.sim.movers_tape_id is not None
    obs = env.reset()
    for _ in range(4):
        obs, rew, done, arrive = env.step(torch.full((32, 2), 0.5, device=DEV))
    assert torch.isfinite(obs.float()).all()
    env.reset()
    held_out = dict(name="random:4", seed=1)
    cfg = ppo.PPOConfig(rollout_len=16, max_episode_steps=30, n_updates_per_iteration=2, policy="mlp64x2", seed=1, eval_every=1,
                        eval_episodes=8, eval_movers=held_out, output_dir=str(tmp_path))
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.uses_persistent_rollout
    for _ in range(2):
        lg = tr.iteration()
        assert np.isfinite([lg["actor_loss"], lg["critic_loss"]]).all(), lg
        assert 0.0 <= lg["eval_scenario_success_min"] <= lg["eval_scenario_success_mean"] <= 1.0
    ev = tr._eval_env
    train_bank, eval_bank = maps.random_mover_bank(4, seed=0)[0], maps.random_mover_bank(4, seed=1)[0]
    assert ev.world_args["movers"] == held_out and env.world_args["movers"] == "random:4"
    np.testing.assert_array_equal(env.sim._mov_tape.cpu().numpy(), train_bank)    # (NaN padding compares equal to itself here)
    np.testing.assert_array_equal(ev.sim._mov_tape.cpu().numpy(), eval_bank)
    assert ev.sim._mov_tape.shape != env.sim._mov_tape.shape or not np.array_equal(train_bank, eval_bank, equal_nan=True)
    env.close()
    ev.close()
