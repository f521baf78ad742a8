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
