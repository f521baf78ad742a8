"""Moving obstacles, the parts that need no GPU: the new entry point is exported and bound (ABI version unchanged), the authored
tapes of navbot_ppo_amd.maps are what their closed form says, and the per-env phase offsets depend on the global env id only."""
import ctypes
import math

import numpy as np
import pytest

from navbot_ppo_amd import maps


def test_library_exports_and_binds_set_movers():
    from navbot_ppo_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(L, "navsim_set_movers")
    bound = {n: (res, args) for n, res, args in _native.SYMBOLS}
    assert "navsim_set_movers" in bound
    res, args = bound["navsim_set_movers"]
    assert res is ctypes.c_int and len(args) == 6 and args[2] is ctypes.c_int32 and args[3] is ctypes.c_int32
    assert L.navsim_version() == _native.NAVSIM_ABI_VERSION == 6   # one more entry point, the same ABI version
    # without a handle the call is refused, with a message, before anything touches a device
    fn = _native.lib().navsim_set_movers
    assert fn(None, None, 0, 0, None, None) == -1 and b"navsim_set_movers" in _native.lib().navsim_last_error()


@pytest.mark.parametrize("period,n,sides", [(1, 4, 8), (7, 4, 8), (40, 3, 6)])
def test_orbit_movers_is_its_closed_form(period, n, sides):
    R, r, c = 1.0, 0.15, (0.25, -0.5)
    tape = maps.orbit_movers(period, n=n, orbit_radius=R, radius=r, sides=sides, centre=c)
    assert tape.shape == (period, n * sides, 4) and tape.dtype == np.float32 and np.isfinite(tape).all()
    for p in {0, period // 2, period - 1}:
        want = []
        for k in range(n):
            a = 2 * math.pi * (p / period + k / n)
            cx, cy = c[0] + R * math.cos(a), c[1] + R * math.sin(a)
            v = [(cx + r * math.cos(2 * math.pi * j / sides), cy + r * math.sin(2 * math.pi * j / sides)) for j in range(sides)]
            want += [[*v[j], *v[(j + 1) % sides]] for j in range(sides)]
        np.testing.assert_array_equal(tape[p], np.asarray(want, np.float64).astype(np.float32))
    # periodic: the frame one period on is the frame itself, and frame `period` closes on frame 0 geometrically (2 pi later)
    for p in (0, period - 1):
        np.testing.assert_array_equal(maps.orbit_frame(p + period, period, n, R, r, sides, c), maps.orbit_frame(p, period, n, R, r, sides, c))
    a = 2 * math.pi
    np.testing.assert_allclose(tape[0, 0, :2], [c[0] + R * math.cos(a) + r, c[1] + R * math.sin(a)], atol=1e-6)
    # every pillar centre sits on the orbit
    ctr = tape.reshape(period, n, sides, 4)[..., :2].astype(np.float64).mean(axis=2)
    np.testing.assert_allclose(np.hypot(ctr[..., 0] - c[0], ctr[..., 1] - c[1]), R, atol=1e-6)


def test_mover_tape_rounds_once_and_checks_its_shape():
    f = np.random.default_rng(0).uniform(-3, 3, (5, 3, 4))
    t = maps.mover_tape(f)
    assert t.dtype == np.float32 and t.shape == (5, 3, 4)
    np.testing.assert_array_equal(t, f.astype(np.float32))
    f[2, 1] = np.nan   # the documented padding survives
    assert np.isnan(maps.mover_tape(f)[2, 1]).all()
    with pytest.raises(ValueError):
        maps.mover_tape(np.zeros((5, 4)))


def test_named_movers_and_the_vecenv_argument_forms():
    t = maps.movers_by_name("orbit4", 12)
    np.testing.assert_array_equal(t, maps.orbit_movers(12, n=4))
    assert maps.movers_by_name("orbit4").shape == (maps.MOVERS_DEFAULT_PERIOD, 32, 4)
    with pytest.raises(KeyError):
        maps.movers_by_name("nope")
    tape, phase = maps.resolve_movers("orbit4")
    assert tape.shape[0] == maps.MOVERS_DEFAULT_PERIOD and phase == "random"
    tape, phase = maps.resolve_movers(dict(name="orbit4", period=9, phase="zero"))
    assert tape.shape == (9, 32, 4) and phase == "zero"
    tape, phase = maps.resolve_movers(t)
    assert tape is t and phase == "random"
    tape, phase = maps.resolve_movers(dict(tape=t, phase="zero"))
    assert tape is t and phase == "zero"
    for bad in (dict(tape=t, name="orbit4"), dict(phase="zero"), dict(tape=t, phase="sometimes"), dict(tape=t, speed=2)):
        with pytest.raises(ValueError):
            maps.resolve_movers(bad)


@pytest.mark.parametrize("period", [1, 7, 40, 65536])
def test_random_phases_depend_on_the_global_env_id_only(period):
    whole = maps.mover_phases(period, 64, map_seed=3, env_id_base=0)
    halves = np.concatenate([maps.mover_phases(period, 32, map_seed=3, env_id_base=0),
                             maps.mover_phases(period, 32, map_seed=3, env_id_base=32)])
    np.testing.assert_array_equal(whole, halves)
    assert whole.dtype == np.int32 and whole.min() >= 0 and whole.max() < period
    if period >= 7:
        assert len(set(whole.tolist())) >= min(period, 64) // 2          # spread over the cycle, not one value
        assert (whole != maps.mover_phases(period, 64, map_seed=4)).any()   # ... and keyed by the map seed


def test_main_has_the_movers_flags():
    from navbot_ppo_amd import main
    a = main.get_args(["--movers", "orbit4", "--movers_period", "20"])
    assert a.movers == "orbit4" and a.movers_period == 20
    a = main.get_args([])
    assert a.movers is None and a.movers_period is None


# ---------------------------------------------------------------- the helpers of tests/test_gpu_movers_edges.py check themselves
def test_tripwire_rows_are_seen_by_every_beam_and_the_interior_is_the_tape():
    from _movers import blade_tape, embed_with_tripwires, tripwire_rows
    from oracle import navsim_oracle as O
    for M in (4, 5, 40):
        wire = tripwire_rows(M)
        assert wire.shape == (M, 4) and wire.dtype == np.float32
        scan = O.raycast(wire, 0.0, 0.0, 0.0)
        assert scan.shape == (10,) and (scan >= 0.3).all() and (scan < 0.4).all()   # all 10 beams, nearer than any blade of the tests
        tape = blade_tape(7, M if M != 40 else 37, pad_to=40 if M == 40 else None, radius=0.45)
        whole = embed_with_tripwires(tape)
        assert whole.shape == (9, M, 4) and whole.dtype == np.float32 and whole.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(whole[1:8], tape)                             # NaN padding included, bit for bit
        assert whole[1:8].tobytes() == tape.tobytes()
        np.testing.assert_array_equal(whole[0], wire)
        np.testing.assert_array_equal(whole[8], wire)
        # ... and the wall changes the scan the tape alone gives at the spawn pose, in every beam
        fin = tape[0][np.isfinite(tape[0]).all(axis=1)]
        assert (O.raycast(np.concatenate([fin, wire]), 0.0, 0.0, 0.0) != O.raycast(fin, 0.0, 0.0, 0.0)).all()


@pytest.mark.parametrize("M", [5, 37, 64])
def test_below_min_poses_face_a_tape_segment_and_no_static_one(M):
    from _movers import LIDAR_X, RANGE_MIN, below_min_poses, blade_tape
    from oracle import navsim_oracle as O
    tape = blade_tape(7, M, pad_to=40 if M == 37 else None)
    phases = np.arange(40) % 7
    pose = below_min_poses(tape, phases)
    assert pose.shape == (40, 3)
    static = maps.stage_1()
    for p, ph in zip(pose, phases):
        ox, oy = p[0] + LIDAR_X * math.cos(p[2]), p[1] + LIDAR_X * math.sin(p[2])
        seg = tape[ph][np.isfinite(tape[ph]).all(axis=1)].astype(np.float64)
        a, e = seg[:, :2], seg[:, 2:] - seg[:, :2]
        t = np.clip(((np.array([ox, oy]) - a) * e).sum(1) / (e * e).sum(1), 0, 1)
        d = np.hypot(*(a + t[:, None] * e - [ox, oy]).T)
        assert d.min() < RANGE_MIN - 0.04                        # the sensor is 7 cm from a tape segment ...
        assert (O.raycast(static, *p) > 1.0).all()               # ... over a metre from every static one in sight,
        assert O.raycast(seg, *p)[4:6].max() == np.float32(RANGE_MIN)   # and the beams beside straight ahead end on the tape below range_min
        assert (O.raycast(seg, *p) >= np.float32(RANGE_MIN)).all()      # (orc_raycast clamps a nearer hit to range_min)


def test_partial_nan_tape_has_one_nan_per_marked_segment():
    from _movers import blade_tape, blade_tape_m1, partial_nan_tape
    tape, whole = partial_nan_tape(7, 12)
    assert tape.shape == whole.shape == (7, 12, 4) and np.isfinite(whole).all()
    nan = np.isnan(tape)
    assert (nan.sum(axis=2)[:, [0, 1, 10, 11]] == 1).all() and not nan[:, 2:10].any()
    assert sorted(np.argwhere(nan[0])[:, 1].tolist()) == [0, 1, 2, 3]               # one in each of the four positions
    np.testing.assert_array_equal(tape[~nan], whole[~nan])
    np.testing.assert_array_equal(tape[:, 2:10], blade_tape(7, 8))
    np.testing.assert_array_equal(blade_tape_m1(64), blade_tape(64, 1))
    big = blade_tape_m1(65536)
    assert big.shape == (65536, 1, 4) and big.nbytes == 1 << 20 and np.isfinite(big).all()


def test_watching_oracle_tells_a_tape_in_sight_from_one_out_of_sight():
    from _movers import MoverOracle, blade_tape
    near = MoverOracle(3, maps.stage_1(), blade_tape(7, 5), watch=True, seed=1)
    far = MoverOracle(3, maps.stage_1(), blade_tape(7, 5) + np.float32(100.0), watch=True, seed=1)
    for s in (near, far):
        s.reset()
        s.step(np.zeros((3, 2), np.float32))
    assert near.seen == [True] and far.seen == [False]
    assert near.tape_in_scan().all() and not far.tape_in_scan().any()


@pytest.mark.parametrize("opts", [dict(), dict(lidar_noise_sigma=0.02), dict(lidar_noise_sigma=0.02, lidar_below_min="gazebo")], ids=str)
def test_mover_oracle_on_a_tape_out_of_sight_is_the_auto_resetting_oracle(opts):
    """MoverOracle steps without auto_reset and resets by a call of its own; with the tape far away that must be, bit for bit, the
    OracleSim with auto_reset on the static map -- the sensor noise of the reset rows included (the in-step auto-reset re-uses the
    step's noise draws: OracleSim.reset(noise_key=...))."""
    from _movers import MoverOracle, blade_tape
    from oracle import navsim_oracle as O
    N, T = 12, 40
    rng = np.random.default_rng(5)
    acts = np.stack([rng.uniform(0.5, 1, (T, N)), rng.uniform(-1, 1, (T, N))], 2).astype(np.float32)
    a = MoverOracle(N, maps.stage_1(), blade_tape(7, 5) + np.float32(100.0), np.arange(N) % 7, max_episode_steps=6, seed=2, **opts)
    b = O.OracleSim(N, max_episode_steps=6, auto_reset=True, seed=2, **opts)
    b.set_map(np.concatenate([maps.stage_1(), blade_tape(7, 5)[0] + np.float32(100.0)]))
    np.testing.assert_array_equal(a.reset(), b.reset())
    ends = 0
    for t in range(T):
        oa, ob = a.step(acts[t]), b.step(acts[t])
        for k in ("obs", "reward", "done", "arrive", "ended"):
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=f"{k}, step {t}")
        ends += int(ob["ended"].sum())
    assert ends >= 6 * N
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k])
