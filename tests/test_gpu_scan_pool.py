"""Sector LiDAR (navsim_set_scan_pool): the simulator casts 10 k rays, each of the 10 scan columns is the nearest return of k
consecutive rays, everything downstream keeps its shape.

A pooled env IS the oracle's env with 10 k beams whose rows go through the reference's Pick(., k), so every check has an exact
reference that already exists: OracleSim / MoverOracle at n_beams = 10 k with their rows pooled (tests/_scan_pool.PooledOracle), and
for the persistent forms the per-step entry points on the same pooled handle."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import test_gpu_continue_rollouts as CR
import test_gpu_evaluate as EV
import test_gpu_scan_history as SH
from _movers import MoverOracle, below_min_poses, blade_tape
from _scan_pool import (ACT_SEED, FIELDS, STEP_BASE, VAR, P, PooledOracle, _st, assert_same_rollout, bits, buffers, dense_raycast,
                        gpu_sim, kernel_rollout16, run_both, same, stepping_rollout16)
from navbot_ppo_amd import maps, nets, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, NavsimError, VecEnv, pool_scan_reference
from oracle import navsim_oracle as O
from test_gpu_parity import OBS_ATOL, _actions, _lockstep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_LOCK = 40   # two full 16-env workgroups and a ragged one of 8
R_NEAR = 0.45   # blades that a robot capped at 9 steps reaches (tests/test_gpu_movers.py)


def _tape(P_, M, radius=0.75):
    return blade_tape(P_, M, pad_to=40 if M == 37 else None, radius=radius)


def _phase0(P_, M, N):
    return np.random.default_rng(1000 * P_ + M).integers(0, P_, N).astype(np.int32)


def _oracle(N, k, map_name, tape=None, ph0=None, **kw):
    """the reference of a handle with scan_pool = k (k = 1: the 10-beam oracle itself)"""
    cpu = PooledOracle(N, k, maps.by_name(map_name), tape, ph0, **kw)
    rr, rs = maps.goal_rects(map_name)
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    return cpu


def _check_info(gpu, k, map_name):
    inf = gpu.info()
    cast = 3 if map_name == "stage_2" else 0
    assert inf["scan_pool"] == k == gpu.scan_pool, inf
    for e in ("step", "seq", "rollout"):
        assert (inf[e + "_epb"], inf[e + "_waves"], inf[e + "_cast"]) == (16, 8, cast), inf
    assert inf["rollout_kind"] == 1 and inf["step_vgprs"] > 0 and inf["step_lds_bytes"] > 0, inf


# ---------------------------------------------------------------- 1. + 3. lock step on static maps, and the share of exact rows
@functools.lru_cache(maxsize=None)
def _static_actions():
    return _actions(np.random.default_rng(31), 200, N_LOCK)


@functools.lru_cache(maxsize=None)
def _static_leg(map_name, k):
    kw = dict(max_episode_steps=90, auto_reset=True, seed=5)
    gpu = gpu_sim(N_LOCK, map_name, k, **kw)
    if k > 1:
        _check_info(gpu, k, map_name)
    st = _lockstep(gpu, _oracle(N_LOCK, k, map_name, **kw), _static_actions())   # flags exact, observations OBS_ATOL, state checks
    gpu.close()
    return st


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("map_name", ["stage_1", "stage_4", "stage_2"])   # 32 segments (several envs per pass), 64 (one tile), tile boxes
def test_lockstep_static_maps(map_name, k):
    st, st1 = _static_leg(map_name, k), _static_leg(map_name, 1)
    share, share1 = st["exact_obs"] / st["total"], st1["exact_obs"] / st1["total"]
    print(f"scan_pool static {map_name} k={k}: done {st['done']} arrive {st['arrive']} ended {st['ended']} "
          f"exact rows {share:.4f} (k=1 leg: done {st1['done']}, exact rows {share1:.4f})")
    assert st["done"] >= 10
    # each column holds up to four near-equal rays whose minimum can flip in the last bit: the parent's share minus one point
    assert share >= share1 - 0.01


# ---------------------------------------------------------------- 2. + 3. lock step with movers
@functools.lru_cache(maxsize=None)
def _mover_actions():
    return _actions(np.random.default_rng(31), 60, N_LOCK)


@functools.lru_cache(maxsize=None)
def _mover_leg(P_, M, k):
    kw = dict(max_episode_steps=25, auto_reset=True, seed=5)
    tape, ph0 = _tape(P_, M), _phase0(P_, M, N_LOCK)
    gpu = gpu_sim(N_LOCK, "stage_1", k, tape, ph0, **kw)
    if k > 1:
        _check_info(gpu, k, "stage_1")
    st = _lockstep(gpu, _oracle(N_LOCK, k, "stage_1", tape, ph0, **kw), _mover_actions())
    gpu.close()
    return st


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("P_,M", [(1, 1), (7, 37), (7, 64)])
def test_lockstep_movers(P_, M, k):
    st, st1 = _mover_leg(P_, M, k), _mover_leg(P_, M, 1)
    share, share1 = st["exact_obs"] / st["total"], st1["exact_obs"] / st1["total"]
    print(f"scan_pool movers P={P_} M={M} k={k}: done {st['done']} ended {st['ended']} exact rows {share:.4f} "
          f"(k=1 leg: done {st1['done']}, exact rows {share1:.4f})")
    assert st["done"] >= 10
    assert share >= share1 - 0.01


# ---------------------------------------------------------------- 4. the blind spot
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_blind_spot_straight_ahead(k):
    """stage_1 plus a 0.15 m square 1.0 m dead ahead of the spawn pose: 10 and 20 beams pass it by (the centre columns read the wall
    behind it), 30 and 40 rays pooled to 10 see it"""
    h = 0.075
    sq = np.array([[1 - h, -h, 1 + h, -h], [1 + h, -h, 1 + h, h], [1 + h, h, 1 - h, h], [1 - h, h, 1 - h, -h]], np.float32)
    seg = np.concatenate([maps.stage_1(), sq])
    g = NavSim(3, device=DEV, scan_pool=k)
    g.set_map(seg)
    io = g.alloc_io()
    row = g.reset(io.obs).cpu().numpy()[0, :10] * 3.5
    ray = g.raycast(torch.zeros((3, 3), dtype=torch.float64)).cpu().numpy()[0]
    want = dense_raycast(seg, (0.0, 0.0, 0.0), k)
    print(f"blind spot k={k}: centre columns {ray[4]:.3f} {ray[5]:.3f} (oracle {want[4]:.3f} {want[5]:.3f})")
    np.testing.assert_allclose(ray, want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(row, np.where(np.isinf(want), 3.5, want), rtol=0, atol=4e-6)
    if k <= 2:
        assert 1.9 < ray[4] < 2.0 and 1.9 < ray[5] < 2.0          # the wall (1.962 / 1.939 m)
    else:
        assert 0.95 < ray[4] < 0.97 and 0.95 < ray[5] < 0.97      # the square (0.958 m)
    g.close()


# ---------------------------------------------------------------- 5. sensor options
SENS = dict(lidar_noise_sigma=0.01, lidar_below_min="gazebo")


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_sensor_options_lockstep(with_tape):
    """noise per dense ray (keyed as the 40-beam oracle keys its beams) and -inf below range_min, k = 4"""
    kw = dict(max_episode_steps=25, auto_reset=True, seed=7, **SENS)
    tape, ph0 = (_tape(7, 37), _phase0(7, 37, N_LOCK)) if with_tape else (None, None)
    gpu = gpu_sim(N_LOCK, "stage_1", 4, tape, ph0, **kw)
    st = _lockstep(gpu, _oracle(N_LOCK, 4, "stage_1", tape, ph0, **kw), _mover_actions())
    gpu.close()
    print(f"scan_pool sensor options tape={with_tape}: done {st['done']} ended {st['ended']} exact rows {st['exact_obs']}/{st['total']}")
    assert st["ended"] >= N_LOCK


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_below_min_readings_win_the_minimum(with_tape):
    N, k = 8, 4
    kw = dict(seed=3, **SENS)
    if with_tape:
        tape, ph0 = _tape(7, 37), _phase0(7, 37, N)
        pose = below_min_poses(tape, (1 + ph0) % 7)   # the phase the step casts (step counter 0)
    else:
        tape = ph0 = None
        pose = np.tile(np.array([[1.9 - 0.06 + 0.032, 0.0, 0.0]]), (N, 1))   # nose-first at stage_1's inner box
        pose[:, 1] = np.linspace(-0.5, 0.5, N)
    gpu = gpu_sim(N, "stage_1", k, tape, ph0, **kw)
    cpu = _oracle(N, k, "stage_1", tape, ph0, **kw)
    io = gpu.alloc_io()
    gpu.reset(io.obs)
    cpu.reset()
    for s in (gpu, cpu):
        s.set_state(pose=pose, goal=np.full((N, 2), 3.0), past_dist=np.full(N, 3.0))
    a = np.zeros((N, 2), np.float32)
    gpu.step(torch.from_numpy(a).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
    out = cpu.cpu.step(a, auto_reset=False) if with_tape else cpu.cpu.step(a)
    want = pool_scan_reference(out["obs"], k)
    og = io.obs.cpu().numpy()
    assert np.isneginf(og[:, :10]).any(axis=1).all() and not io.done.any()
    np.testing.assert_array_equal(np.isneginf(og), np.isneginf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(og[fin], want[fin], rtol=0, atol=OBS_ATOL)
    np.testing.assert_array_equal(io.done.cpu().numpy(), out["done"])
    gpu.close()


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_float16_rows_are_the_rounded_float32_rows(with_tape):
    N, T, k = N_LOCK, 40, 4
    kw = dict(max_episode_steps=9, auto_reset=True, seed=7, **SENS)
    tape, ph0 = (_tape(7, 37, R_NEAR), _phase0(7, 37, N)) if with_tape else (None, None)
    a, b = gpu_sim(N, "stage_1", k, tape, ph0, obs_f16=True, **kw), gpu_sim(N, "stage_1", k, tape, ph0, **kw)
    ia, ib = a.alloc_io(), b.alloc_io()
    assert ia.obs.dtype == torch.float16 and same(a.reset(ia.obs), b.reset(ib.obs).half())
    acts = torch.from_numpy(_actions(np.random.default_rng(45), T, N)).to(DEV)
    for t in range(T):
        a.step(acts[t], ia.obs, ia.reward, ia.done, ia.arrive, ia.ended)
        b.step(acts[t], ib.obs, ib.reward, ib.done, ib.arrive, ib.ended)
        assert same(ia.obs, ib.obs.half()), t
        for f in ("reward", "done", "arrive", "ended"):
            assert same(getattr(ia, f), getattr(ib, f)), (f, t)
    a.close()
    b.close()


# ---------------------------------------------------------------- 6. persistent forms against per-step launches
K6, T6, CAP6 = 3, 30, 9


def _sim6(with_tape, n=N_LOCK, k=K6, cap=CAP6, **kw):
    tape, ph0 = (_tape(7, 32, R_NEAR), _phase0(7, 32, n)) if with_tape else (None, None)
    return gpu_sim(n, "stage_1", k, tape, ph0, max_episode_steps=cap, auto_reset=True, seed=8, **kw)


@functools.lru_cache(maxsize=None)
def _actor16():
    return EV._actor("mlp64x2", 16)[1]


def _step_seq_vs_steps(a, b, T, place=None):
    N = a.N
    acts = torch.from_numpy(_actions(np.random.default_rng(45), T, N)).to(DEV)
    ia, ib = a.alloc_io(), b.alloc_io()
    assert same(a.reset(ia.obs), b.reset(ib.obs))
    mk = place or (lambda shape, dt, align: torch.zeros(shape, dtype=dt, device=DEV))
    z = lambda dt, align, *s: mk((T, N) + s, dt, align)
    seq = dict(obs=z(a.obs_dtype, 16, 16), reward=z(torch.float32, 4), done=z(torch.uint8, 1), arrive=z(torch.uint8, 1),
               ended=z(torch.uint8, 1))
    stats = {f: torch.zeros((T, N), dtype=dt, device=DEV) for f, dt in (("ep_return", torch.float32), ("ep_length", torch.int32),
                                                                          ("ep_path", torch.float32))}
    a.step_seq(acts, seq["obs"], seq["reward"], seq["done"], seq["arrive"], seq["ended"], stats["ep_return"], stats["ep_length"],
               stats["ep_path"])
    for t in range(T):
        b.step(acts[t], ib.obs, ib.reward, ib.done, ib.arrive, ib.ended, ib.ep_return, ib.ep_length, ep_path=ib.ep_path)
        for f in ("obs", "reward", "done", "arrive", "ended"):
            assert same(seq[f][t], getattr(ib, f)), (f, t)
        e = ib.ended.bool()
        for f in stats:
            assert same(stats[f][t][e], getattr(ib, f)[e]), (f, t)
    sa, sb = a.get_state(), b.get_state()
    for f in sa:
        np.testing.assert_array_equal(sa[f], sb[f])
    return seq


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_step_seq_equals_step_launches(with_tape):
    a, b = _sim6(with_tape), _sim6(with_tape)
    seq = _step_seq_vs_steps(a, b, T6)
    assert int(seq["ended"].sum()) > 2 * N_LOCK and (not with_tape or int(seq["done"].sum()) > 0)
    a.close()
    b.close()

    def call(g):   # once more with every output inside a guarded allocation
        a, b = _sim6(with_tape), _sim6(with_tape)
        try:
            return _step_seq_vs_steps(a, b, T6, place=lambda shape, dt, align: g.out(shape, dt, align))
        finally:
            a.close()
            b.close()
    got = run_both(DEV, call, "navsim_step_seq pooled")
    for f in seq:
        assert same(got[f], seq[f]), f


def _guarded_rollout(entry, make, flat, T, start, carries=False):
    """the rollout entry point with every argument inside a guarded allocation (tests/test_gpu_scan_history.py's placement)"""
    def call(g):
        s = make()
        try:
            b = buffers(s, T, place=g.out, place_stats=g.io)
            start(s, b["obs"][0])
            pr, var = g.inp(flat, 16), g.inp(torch.tensor([VAR], device=DEV), 4)
            base = g.inp(torch.tensor([STEP_BASE], dtype=torch.int32, device=DEV), 4)
            extra = ()
            if carries:
                cout = g.out((s.N, 22), torch.float32, 16)
                extra = (None, P(cout))
            rc = getattr(lib(), entry)(s._h, P(pr), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]), P(b["arrive"]),
                                       P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var), ACT_SEED, P(base), T,
                                       *extra, _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            return {f: b[f].clone() for f in FIELDS}
        finally:
            s.close()
    return run_both(DEV, call, entry + " pooled")


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_rollout_mlp64_equals_the_stepping_loop(with_tape):
    flat = _actor16()
    a, b = _sim6(with_tape), _sim6(with_tape)
    got, gs = kernel_rollout16(a, flat, T6)
    want, ws = stepping_rollout16(b, flat, T6)
    a.close()
    b.close()
    assert int(want["ended"].sum()) > 2 * N_LOCK
    assert_same_rollout(got, gs, want, ws, f"navsim_rollout_mlp64 tape={with_tape}")
    guarded = _guarded_rollout("navsim_rollout_mlp64", lambda: _sim6(with_tape), flat, T6, lambda s, obs0: s.reset(obs0))
    for f in FIELDS:
        assert same(guarded[f], got[f]), f


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_rollout_hist_and_hist_cont_equal_the_stepping_loop(with_tape):
    flat = SH._actor()[1]
    a, b, c = _sim6(with_tape), _sim6(with_tape), _sim6(with_tape)
    got, gs = SH.kernel_rollout(a, flat, T6)          # navsim_rollout_mlp64_hist
    want, ws = SH.stepping_rollout(b, flat, T6)       # HistoryWindow (navsim_stack_rows) -> navppo_mlp64_act(42) -> navsim_step
    # navsim_rollout_mlp64_hist_cont in three pieces: a carry out of the first, in and out of the second, into the third
    cont, carry = CR.chained("navsim_rollout_mlp64_hist_cont", c, flat, [7, 19], T6, cont=True, inplace=False, start=SH.start)
    cs = c.get_state()
    for s in (a, b, c):
        s.close()
    assert int(want["ended"].sum()) > 2 * N_LOCK
    assert_same_rollout(got, gs, want, ws, f"navsim_rollout_mlp64_hist tape={with_tape}")
    assert_same_rollout(cont, cs, want, ws, f"navsim_rollout_mlp64_hist_cont tape={with_tape}")
    assert same(carry, CR.mirror_carry(want))
    guarded = _guarded_rollout("navsim_rollout_mlp64_hist_cont", lambda: _sim6(with_tape), flat, T6, SH.start, carries=True)
    for f in FIELDS:
        assert same(guarded[f], got[f]), f


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
@pytest.mark.parametrize("hist", [False, True], ids=["mlp64", "hist"])
def test_evaluation_table_equals_the_stepping_loop(hist, with_tape):
    quota = 2
    tabs = []
    for kernel in (False, True):
        s = _sim6(with_tape, threshold_arrive=0.4)
        if hist:
            fn = SH.kernel_table_hist if kernel else SH.reference_table_hist
            r = fn(s, SH._actor()[1], quota, quota * CAP6)
        else:
            fn = EV.kernel_table if kernel else EV.reference_table
            r = fn(s, "mlp64x2", _actor16(), quota, quota * CAP6)
        tabs.append(r[0] if isinstance(r, tuple) else r)
        s.close()
    want, got = tabs
    assert (want["count"] == quota).all()
    EV.assert_tables_equal(got, want, f"pooled evaluate hist={hist} tape={with_tape}")

    def call(g):   # once more inside guarded allocations
        s = _sim6(with_tape, threshold_arrive=0.4)
        try:
            n = s.N
            obs0 = g.out((n, 16), s.obs_dtype, 16)
            s.reset(obs0)
            pr = g.inp(SH._actor()[1] if hist else _actor16(), 16)
            fl = g.out((quota, n), torch.uint8, 1)
            ln, rt, pa = g.out((quota, n), torch.int32, 4), g.out((quota, n), torch.float32, 4), g.out((quota, n), torch.float32, 4)
            cnt, stp = g.out((n,), torch.int32, 4), g.out(((n + 15) // 16,), torch.int32, 4)
            entry = lib().navsim_evaluate_mlp64_hist if hist else lib().navsim_evaluate_mlp64
            rc = entry(s._h, P(pr), P(obs0), quota, quota * CAP6, P(fl), P(ln), P(rt), P(pa), P(cnt), P(stp), _st())
            assert rc == 0, lib().navsim_last_error().decode()
            torch.cuda.synchronize()
            return dict(flags=fl.cpu().numpy(), length=ln.cpu().numpy(), ret=rt.cpu().numpy(), path=pa.cpu().numpy(),
                        count=cnt.cpu().numpy(), steps=stp.cpu().numpy())
        finally:
            s.close()
    EV.assert_tables_equal(run_both(DEV, call, "pooled evaluate"), want, "guarded")


# ---------------------------------------------------------------- 7. set_scan_pool(1) after set_scan_pool(4); call order
def _rows(g, T=30):
    acts = torch.from_numpy(_actions(np.random.default_rng(47), T, g.N)).to(DEV)
    io = g.alloc_io()
    rows = [g.reset(io.obs).clone()]
    for t in range(T):
        g.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
        rows += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.arrive.clone(), io.ended.clone()]
    return rows


@pytest.mark.parametrize("map_name", ["stage_1", "stage_2"])
def test_pool_1_after_pool_4_is_a_fresh_handle(map_name):
    kw = dict(max_episode_steps=9, auto_reset=True, seed=2)
    fresh = gpu_sim(N_LOCK, map_name, 1, **kw)
    back = gpu_sim(N_LOCK, map_name, 4, **kw)
    gen = back.generation
    assert back.info()["scan_pool"] == 4
    back.set_scan_pool(1)
    assert back.generation == gen + 1 and back.scan_pool == 1
    assert back.info() == fresh.info() and fresh.info()["scan_pool"] == 1
    assert all(same(x, y) for x, y in zip(_rows(back), _rows(fresh)))
    fresh.close()
    back.close()


@pytest.mark.parametrize("with_tape", [False, True], ids=["static", "tape"])
def test_pool_before_or_after_the_world_gives_the_same_bits(with_tape):
    kw = dict(max_episode_steps=9, auto_reset=True, seed=2, lidar_noise_sigma=0.01)
    tape, ph0 = (_tape(7, 32, R_NEAR), _phase0(7, 32, N_LOCK)) if with_tape else (None, None)
    a = gpu_sim(N_LOCK, "stage_1", 3, tape, ph0, pool_first=True, **kw)
    b = gpu_sim(N_LOCK, "stage_1", 3, tape, ph0, pool_first=False, **kw)
    assert a.info() == b.info()
    ra, rb = _rows(a), _rows(b)
    assert all(same(x, y) for x, y in zip(ra, rb))
    a.set_map(maps.stage_4())   # a later set_map keeps the pool (and the tape): the spawn scans are re-cast for the dense fan
    assert a.info()["scan_pool"] == 3 and a.info()["n_segments"] == len(maps.stage_4())
    a.close()
    b.close()


def test_vecenv_and_trainer_follow_the_handles_scan_pool():
    env = VecEnv(16, map="stage_1", max_episode_steps=9, seed=1)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=4, max_episode_steps=9, policy="mlp64x2"))
    assert env.scan_pool == 1 and "scan_pool" not in env.world_args and tr.scan_pool == 1
    env.set_scan_pool(3)
    assert env.scan_pool == 3 and env.world_args["scan_pool"] == 3 and tr.scan_pool == 3 and env.sim.info()["scan_pool"] == 3
    env.sim.set_scan_pool(2)   # ... and the handle's own call
    assert env.scan_pool == 2 and env.world_args["scan_pool"] == 2 and tr.scan_pool == 2
    env.sim.set_scan_pool(1)
    assert env.scan_pool == 1 and "scan_pool" not in env.world_args
    env.close()


# ---------------------------------------------------------------- 8. shards
def test_shards_equal_the_whole():
    """envs 0..23 and 24..39 under env_id_base equal the 40-env handle: phase="random" movers and the noise key follow the global id"""
    T, k = 30, 4
    acts = torch.from_numpy(_actions(np.random.default_rng(49), T, N_LOCK)).to(DEV)
    outs = {}
    for lo, hi in ((0, 40), (0, 24), (24, 40)):
        env = VecEnv(hi - lo, map="stage_1", max_episode_steps=9, seed=3, map_seed=5, env_id_base=lo, lidar_noise_sigma=0.01,
                     movers=dict(tape=_tape(7, 32, R_NEAR), phase="random"), scan_pool=k)
        assert env.sim.info()["scan_pool"] == k
        rows = [env.reset().clone()]
        for t in range(T):
            env.step(acts[t, lo:hi])
            rows += [env.io.obs.clone(), env.io.reward.clone(), env.io.done.clone(), env.io.ended.clone()]
        outs[(lo, hi)] = rows
        env.close()
    for j, whole in enumerate(outs[(0, 40)]):
        assert same(whole[:24], outs[(0, 24)][j]) and same(whole[24:], outs[(24, 40)][j]), j


# ---------------------------------------------------------------- 9. rounds of workgroups
def test_4117_envs_run_in_rounds_of_workgroups():
    N, T, k = 4117, 4, 2
    flat = _actor16()
    mk = lambda: gpu_sim(N, "stage_1", k, max_episode_steps=3, auto_reset=True, seed=4)
    a, b = mk(), mk()
    inf = a.info()
    assert (inf["rollout_kind"], inf["rollout_epb"], inf["rollout_waves"], inf["step_epb"]) == (1, 16, 8, 16), inf
    got, gs = kernel_rollout16(a, flat, T)
    want, ws = stepping_rollout16(b, flat, T)
    assert_same_rollout(got, gs, want, ws, "4117 envs")
    assert int(want["ended"].sum()) >= N
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. refusals
def _rc(fn, *a):
    return fn(*a), lib().navsim_last_error().decode()


def test_refusals():
    L = lib()
    g = NavSim(32, device=DEV)
    for bad in (0, 5, -1):
        rc, msg = _rc(L.navsim_set_scan_pool, g._h, bad)
        assert rc == -1 and "1, 2, 3 or 4" in msg and "not built" in msg, msg
    assert _rc(L.navsim_set_scan_pool, None, 2)[0] == -1
    assert _rc(L.navsim_set_scan_pool, g._h, 2)[0] == 0          # before a map: fine
    g.set_map(maps.stage_1())
    assert g.info()["scan_pool"] == 2
    rc, msg = _rc(L.navsim_set_map, g._h, P(torch.from_numpy(maps.replicate_per_env(maps.stage_1(), 32)).to(DEV)), 32, 1, None)
    assert rc == -1 and "per-env maps" in msg and "not built" in msg, msg     # a later per-env map on a pooled handle
    assert g.info()["scan_pool"] == 2 and g.info()["per_env_map"] == 0
    assert _rc(L.navsim_set_shape, g._h, 64, -1)[0] == 0                       # accepted, without effect on pooled launches
    inf = g.info()
    assert (inf["step_epb"], inf["step_waves"], inf["rollout_kind"], inf["rollout_epb"]) == (16, 8, 1, 16), inf
    # the 512-wide nets on a pooled handle: the not_built path, nothing launched
    tr_env = VecEnv(32, map="stage_1", max_episode_steps=9, seed=1, scan_pool=2)
    flat = torch.zeros(50290, device=DEV)
    with pytest.raises(NavsimError, match="not built"):
        tr_env.evaluate_policy(flat, 1, policy="resmlp512")
    b = buffers(tr_env.sim, 2)
    var, base = torch.tensor(0.3, device=DEV), torch.tensor(0, dtype=torch.int32, device=DEV)
    rc, msg = _rc(L.navsim_rollout_resmlp512, tr_env.sim._h, P(flat), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                  P(b["arrive"]), P(b["ended"]), None, None, None, P(var), 1, P(base), 2, None)
    assert rc == -3 and "not built" in msg, msg
    tr_env.close()
    g.close()

    g36 = NavSim(32, n_beams=36, device=DEV)
    rc, msg = _rc(L.navsim_set_scan_pool, g36._h, 2)
    assert rc == -1 and "n_beams == 10" in msg and "not built" in msg, msg
    assert _rc(L.navsim_set_scan_pool, g36._h, 1)[0] == 0
    g36.close()

    gp = NavSim(32, device=DEV)
    gp.set_map(maps.replicate_per_env(maps.stage_1(), 32), per_env=True)
    rc, msg = _rc(L.navsim_set_scan_pool, gp._h, 3)
    assert rc == -1 and "per-env maps" in msg and "not built" in msg, msg
    with pytest.raises(ValueError, match="not built"):
        gp.set_scan_pool(3)
    gp.close()

    # the Python layer, at construction
    for bad in (0, 5, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="scan_pool"):
            NavSim(4, device=DEV, scan_pool=bad)
    with pytest.raises(ValueError, match="n_beams == 10"):
        VecEnv(4, n_beams=36, scan_pool=2)
    with pytest.raises(ValueError, match="per-env maps"):
        VecEnv(4, per_env_map=True, scan_pool=2)
    env = VecEnv(16, map="stage_1", max_episode_steps=9, scan_pool=2)
    with pytest.raises(ValueError, match="resmlp512"):
        ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=4, max_episode_steps=9, policy="resmlp512"))
    env.close()


# ---------------------------------------------------------------- 11. the trainer
@pytest.mark.parametrize("scan_history", [False, True], ids=["rows16", "history"])
def test_trainer_on_a_pooled_env(scan_history, tmp_path):
    N, T, k, cap = 64, 32, 4, 30
    env = VecEnv(N, map="stage_1", max_episode_steps=cap, seed=3, movers="orbit4", scan_pool=k)
    cfg = ppo.PPOConfig(rollout_len=T, max_episode_steps=cap, n_updates_per_iteration=2, policy="mlp64x2", seed=1, eval_every=1,
                        eval_episodes=16, output_dir=str(tmp_path), scan_history=scan_history)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.uses_persistent_rollout and tr.scan_pool == k and env.world_args["scan_pool"] == k
    with torch.no_grad():   # drive: a forward bias on the linear-velocity head, so that the robots reach the pillars' orbit
        tr.actor.layer3.bias.add_(2.0)
    tape = np.asarray(maps.movers_by_name("orbit4", None))
    ph0 = env.sim._mov_phase0.cpu().numpy()
    for it in range(2):
        lg = tr.iteration()
        assert np.isfinite([lg["actor_loss"], lg["critic_loss"]]).all() and lg["scan_pool"] == k and "eval_success" in lg
        assert tr.obs_buf.shape == (T + 1, N, 16)
        # the rollout's rows replay on the 40-ray MoverOracle from the recorded actions
        cpu = PooledOracle(N, k, maps.stage_1(), tape, ph0, max_episode_steps=cap, seed=3)
        rr, rs = maps.goal_rects("stage_1")
        cpu.set_goal_rects(0, rr)
        cpu.set_goal_rects(1, rs)
        if it == 0:
            obs, act = tr.obs_buf.float().cpu().numpy(), tr.act_buf.cpu().numpy()
            np.testing.assert_allclose(obs[0], cpu.reset(), rtol=0, atol=OBS_ATOL)
            for t in range(T):
                out = cpu.step(act[t])
                np.testing.assert_allclose(obs[t + 1], out["obs"], rtol=0, atol=OBS_ATOL, err_msg=f"row {t + 1}")
                np.testing.assert_array_equal(tr.done_buf[t].cpu().numpy(), out["done"])
                np.testing.assert_array_equal(tr.ended_buf[t].cpu().numpy(), out["ended"])
    ev = tr._eval_env
    assert ev is not None and ev.sim.scan_pool == k and ev.sim.info()["scan_pool"] == k
    assert tr.tb_scalars()["env/scan_pool"] == k
    env.close()
    ev.close()
