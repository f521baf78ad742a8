"""Env(..., movers=...): what the keyword accepts (navbot_ppo_amd.env.resolve_env_movers), and that the Env test's poses and tape put
the tape into the oracle's scans -- both without a GPU."""
import numpy as np
import pytest

from _movers import MoverOracle, blade_tape
from navbot_ppo_amd import maps
from navbot_ppo_amd.env import resolve_env_movers


def test_a_tape_a_name_or_a_dict():
    tape = blade_tape(7, 5)
    for arg in (tape, tape.astype(np.float64), dict(tape=tape), dict(tape=tape.tolist())):
        t, ph = resolve_env_movers(arg)
        assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and ph == 0
        np.testing.assert_array_equal(t, tape)
    t, ph = resolve_env_movers(dict(tape=tape, phase=6))
    assert ph == 6 and isinstance(ph, int)
    t, ph = resolve_env_movers(dict(tape=tape, phase=np.int32(2)))
    assert ph == 2 and isinstance(ph, int)
    t, ph = resolve_env_movers("orbit4")
    np.testing.assert_array_equal(t, maps.movers_by_name("orbit4"))
    assert ph == 0 and t.shape[0] == maps.MOVERS_DEFAULT_PERIOD
    t, ph = resolve_env_movers(dict(name="orbit4", period=12, phase=11))
    assert t.shape[0] == 12 and ph == 11
    np.testing.assert_array_equal(t, maps.movers_by_name("orbit4", 12))


@pytest.mark.parametrize("bad", [dict(tape=blade_tape(7, 5), phase=7), dict(tape=blade_tape(7, 5), phase=-1),
                                 dict(tape=blade_tape(7, 5), phase="random"), dict(tape=blade_tape(7, 5), phase=1.0),
                                 dict(tape=blade_tape(7, 5), phase=True), dict(tape=blade_tape(7, 5), name="orbit4"), dict(phase=1),
                                 dict(tape=blade_tape(7, 5), period=7), dict(tape=blade_tape(7, 5), bank=1), np.zeros((7, 5, 3), np.float32),
                                 np.zeros((5, 4), np.float32), np.zeros((0, 5, 4), np.float32)])
def test_refused_arguments(bad):
    with pytest.raises(ValueError, match="movers"):
        resolve_env_movers(bad)


def test_unknown_name():
    with pytest.raises(KeyError):
        resolve_env_movers("no-such-scene")


def test_the_phase_rule_of_one_env_across_a_reset():
    """the oracle of tests/test_gpu_movers_big.py's Env test, alone: the phase follows (k + 1 + phase) mod P with k zeroed by a reset,
    and the blades are in most scans along the driven path"""
    P, phase = 7, 3
    tape = blade_tape(P, 5)
    cpu = MoverOracle(1, maps.stage_1(), tape, [phase], respawn_on_arrive=True, threshold_arrive=0.2, seed=0)
    cpu.reset()
    k = seen = 0
    for s in range(30):
        if s == 14:
            cpu.reset()
            k = 0
        assert int(cpu.step_phases()[0]) == (k + 1 + phase) % P
        cpu.step(np.array([[0.9, 0.3 * np.sin(0.7 * s)]], np.float32), auto_reset=False)
        seen += int(cpu.tape_in_scan()[0])
        k += 1
    assert seen > 15
