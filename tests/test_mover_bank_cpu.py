"""CPU-only checks of the mover bank (navsim_set_mover_bank): the arrays maps.mover_bank builds, the per-env tape ids and phases, the
authored scenario generators, every new form of resolve_movers, the per-scenario grouping of evaluate() and the ABI."""
import numpy as np
import pytest

from navbot_ppo_amd import evaluate as ev
from navbot_ppo_amd import maps

START = (0.0, 0.0)      # the stage maps' spawn pose
CLEAR = 0.6             # house()'s clear_radius: no segment of any phase comes closer to a start pose


def test_mover_bank_pads_with_nan_and_keeps_the_periods():
    a, b = maps.orbit_movers(5, n=1, sides=3), maps.clutter_tape([(1.0, 1.0), (2.0, -1.0)], sides=4)
    bank, periods, rects = maps.mover_bank([a, b], [[], maps.clutter_rects([(1.0, 1.0), (2.0, -1.0)])])
    assert bank.dtype == np.float32 and bank.shape == (2, 5, 8, 4) and periods.dtype == np.int32 and periods.tolist() == [5, 1]
    np.testing.assert_array_equal(bank[0, :, :3], a)
    np.testing.assert_array_equal(bank[1, :1], b)
    assert np.isnan(bank[0, :, 3:]).all() and np.isnan(bank[1, 1:]).all()
    assert rects.dtype == np.float64 and rects.shape == (2, 2, 4) and np.isnan(rects[0]).all() and np.isfinite(rects[1]).all()
    bank, periods, rects = maps.mover_bank([a])
    assert bank.shape == (1, 5, 3, 4) and rects.shape == (1, 0, 4)
    for bad in ([], [np.zeros((3, 4))], [np.zeros((2, 0, 4))]):
        with pytest.raises(ValueError):
            maps.mover_bank(bad)
    with pytest.raises(ValueError):
        maps.mover_bank([a, b], [[]])


def test_tape_ids_and_phases_are_shard_invariant_and_in_range():
    K, n = 5, 1000
    ids = maps.mover_tape_ids(K, n, map_seed=3)
    assert ids.dtype == np.int32 and ids.min() == 0 and ids.max() == K - 1 and np.bincount(ids).min() > n / K / 2
    np.testing.assert_array_equal(ids, np.concatenate([maps.mover_tape_ids(K, 400, 3, 0), maps.mover_tape_ids(K, 600, 3, 400)]))
    assert (ids != maps.mover_tape_ids(K, n, map_seed=4)).any()
    assert (maps.mover_tape_ids(1, 50) == 0).all()
    periods = np.array([1, 7, 64, 128, 13], np.int32)
    ph = maps.mover_bank_phases(periods[ids], map_seed=3)
    assert ph.dtype == np.int32 and (ph >= 0).all() and (ph < periods[ids]).all() and (ph[ids == 0] == 0).all()
    np.testing.assert_array_equal(ph, np.concatenate([maps.mover_bank_phases(periods[ids[:400]], 3, 0),
                                                      maps.mover_bank_phases(periods[ids[400:]], 3, 400)]))
    # K = 1: mover_phases; and an env's tape and its phase come from different hashes
    np.testing.assert_array_equal(maps.mover_bank_phases(np.full(n, 64), 3, 17), maps.mover_phases(64, n, 3, 17))
    assert (maps.mover_tape_ids(64, n, 3) != maps.mover_phases(64, n, 3)).any()


def test_mover_phases_is_what_it_was():
    """the hash was factored out for the tape ids: its values are pinned here (computed by the function as it stood before)"""
    assert maps.mover_phases(64, 6, map_seed=0, env_id_base=0).tolist() == [17, 28, 60, 33, 42, 30]
    assert maps.mover_phases(7, 4, map_seed=5, env_id_base=1000).tolist() == [5, 0, 3, 6]


def test_generators_keep_clear_of_the_start_pose_in_every_phase():
    ends = [(1.0, -1.0, 1.0, 1.0), (-2.0, 2.0, 2.0, 2.0)]
    t = maps.patrol_movers(16, ends, radius=0.15, sides=8)
    assert t.shape == (16, 16, 4) and maps.mover_clearance(t, [START]) >= CLEAR
    # one round trip per period: at a at phase 0, at b at half the period, symmetric about it
    centre = lambda fr, k: fr[8 * k:8 * k + 8, :2].astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(centre(t[0], 0), (1.0, -1.0), atol=1e-6)
    np.testing.assert_allclose(centre(t[8], 0), (1.0, 1.0), atol=1e-6)
    np.testing.assert_allclose(centre(t[3], 1), centre(t[13], 1), atol=1e-6)
    for name in ("orbit4", "orbit2", "patrol2", "clutter4"):
        assert maps.mover_clearance(maps.movers_by_name(name), [START]) >= CLEAR, name
    bank, periods, rects = maps.random_mover_bank(32, seed=0)
    assert bank.shape[0] == 32 and bank.shape[2] == 32 and set(periods.tolist()) <= {1, 32, 64, 128} and rects.shape[1] <= 8
    for k in range(32):
        tape = bank[k, :periods[k]]
        assert np.isfinite(tape).all()
        assert maps.mover_clearance(tape, [START]) >= CLEAR, k
        assert np.abs(tape).max() <= 3.6 + 0.15 + 1e-6      # inside the goal box, up to a pillar's radius
    assert (periods == 1).any() and (periods > 1).any()


def test_rectangles_cover_their_clutter():
    c = [(1.0, 2.0), (-2.5, 0.4)]
    r = maps.clutter_rects(c, radius=0.2, margin=0.3)
    t = maps.clutter_tape(c, radius=0.2, sides=8)
    assert t.shape == (1, 16, 4) and r.shape == (2, 4)
    np.testing.assert_allclose(r[0], (0.5, 1.5, 1.5, 2.5))
    for k in range(2):
        pts = t[0, 8 * k:8 * k + 8].reshape(-1, 2)
        assert (pts[:, 0] >= r[k, 0]).all() and (pts[:, 0] <= r[k, 1]).all() and (pts[:, 1] >= r[k, 2]).all() and (pts[:, 1] <= r[k, 3]).all()
    # a random bank: every standing pillar (a polygon that is the same in all phases of its tape) lies inside one of its tape's rectangles
    bank, periods, rects = maps.random_mover_bank(16, seed=3)
    standing = 0
    for k in range(16):
        tape = bank[k, :periods[k]]
        for j in range(0, 32, 8):
            if (tape[:, j:j + 8] == tape[0, j:j + 8]).all():
                pts = tape[0, j:j + 8].reshape(-1, 2)
                rk = rects[k][~np.isnan(rects[k]).any(axis=1)]
                inside = [(pts[:, 0] >= q[0]).all() and (pts[:, 0] <= q[1]).all() and (pts[:, 1] >= q[2]).all() and (pts[:, 1] <= q[3]).all()
                          for q in rk]
                assert any(inside), (k, j)
                standing += 1
    assert standing > 0


def test_random_mover_bank_is_a_pure_function_of_its_seed():
    a, b, c = maps.random_mover_bank(8, seed=0), maps.random_mover_bank(8, seed=0), maps.random_mover_bank(8, seed=1)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[0].shape != c[0].shape or not np.array_equal(a[0], c[0], equal_nan=True)
    # scenario k does not depend on K
    big = maps.random_mover_bank(12, seed=0)
    assert big[1][:8].tolist() == a[1].tolist()
    for k in range(8):
        np.testing.assert_array_equal(big[0][k, :a[1][k]], a[0][k, :a[1][k]])


def test_resolve_movers_new_forms():
    tape, phase = maps.resolve_movers("orbit4")                              # the old forms are what they were
    assert isinstance(tape, np.ndarray) and tape.shape == (64, 32, 4) and phase == "random"
    mb, phase = maps.resolve_movers("random:4")
    assert isinstance(mb, maps.MoverBank) and phase == "random" and mb.assign == "random" and len(mb.periods) == 4
    np.testing.assert_array_equal(mb.bank, maps.random_mover_bank(4, seed=0)[0])
    mb1, phase = maps.resolve_movers(dict(name="random:4", seed=1, phase="zero", assign="cycle"))
    assert phase == "zero" and mb1.assign == "cycle"
    np.testing.assert_array_equal(mb1.bank, maps.random_mover_bank(4, seed=1)[0])
    np.testing.assert_array_equal(mb1.tape_ids(6, env_id_base=3), [3, 0, 1, 2, 3, 0])
    mb2, _ = maps.resolve_movers("bank:orbit4,patrol2,clutter4")
    assert mb2.bank.shape == (3, 64, 32, 4) and mb2.periods.tolist() == [64, 64, 1]
    assert np.isnan(mb2.rects[:2]).all() and np.isfinite(mb2.rects[2]).all() and mb2.rects.shape == (3, 4, 4)
    assert maps.resolve_movers(dict(name="bank:orbit4,patrol2", period=16))[0].periods.tolist() == [16, 16]
    bank, periods, rects = maps.mover_bank([maps.orbit_movers(5, n=1), maps.clutter_tape([(2.0, 2.0)])])
    mb3, _ = maps.resolve_movers(dict(bank=bank, periods=periods, rects=rects, assign=np.array([0, 1, 1, 0])))
    assert mb3.tape_ids(4).tolist() == [0, 1, 1, 0] and mb3.periods.tolist() == [5, 1]
    np.testing.assert_array_equal(maps.resolve_movers(dict(bank=bank))[0].periods, [5, 5])
    ids = maps.resolve_movers(dict(bank=bank, periods=periods))[0].tape_ids(100, map_seed=2, env_id_base=7)
    np.testing.assert_array_equal(ids, maps.mover_tape_ids(2, 100, 2, 7))


@pytest.mark.parametrize("spec,word", [
    (dict(bank=np.zeros((2, 3, 4))), "bank must be"),
    (dict(bank=np.zeros((2, 3, 4, 4)), periods=[3]), "periods"),
    (dict(bank=np.zeros((2, 3, 4, 4)), periods=[3, 4]), "periods"),
    (dict(bank=np.zeros((2, 3, 4, 4)), assign="nearest"), "assign"),
    (dict(bank=np.zeros((2, 3, 4, 4)), tape=np.zeros((3, 4, 4))), "give a bank, a tape or a name"),
    (dict(bank=np.zeros((2, 3, 4, 4)), colour=1), "unknown entries"),
    ("random:0", "random:K"), ("random:x", "random:K"), ("bank:", "lists no scene"), (dict(name="orbit4", phase="late"), "phase"),
])
def test_resolve_movers_error_messages(spec, word):
    with pytest.raises(ValueError, match=word):
        maps.resolve_movers(spec)


def test_resolve_movers_unknown_scene_and_bad_ids():
    with pytest.raises(KeyError, match="unknown movers"):
        maps.resolve_movers("bank:orbit4,waltz")
    mb, _ = maps.resolve_movers(dict(bank=np.zeros((2, 3, 4, 4)), assign=np.array([0, 2, 1])))
    with pytest.raises(ValueError, match="assign"):
        mb.tape_ids(3)
    with pytest.raises(ValueError, match="assign"):
        mb.tape_ids(4)


def test_scenario_report_groups_the_episode_table_by_tape_id():
    # evaluate()'s rows, slot-major: row r was played by env r % 4; columns episode, success, collision, timeout, length, return, path, time
    tape_id = np.array([0, 2, 2, 0])
    outcome = [(1, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 0),      # slot 0 of envs 0..3
               (0, 0, 1), (0, 1, 0), (1, 0, 0)]                 # slot 1 of envs 0..2 (the table was cut to 7 episodes)
    rows = [[r, s, c, t, 10, 1.0, 2.0, 0.1] for r, (s, c, t) in enumerate(outcome)]
    sc = ev.scenario_report(rows, tape_id, 3)
    assert [d["scenario"] for d in sc] == [0, 1, 2] and [d["episodes"] for d in sc] == [3, 0, 4]
    assert sc[0]["success_rate"] == pytest.approx(2 / 3) and sc[0]["timeout_rate"] == pytest.approx(1 / 3) and sc[0]["collision_rate"] == 0
    assert sc[2]["success_rate"] == 0.5 and sc[2]["collision_rate"] == 0.5 and sc[2]["timeout_rate"] == 0
    assert np.isnan(sc[1]["success_rate"])
    mn, mean = ev.scenario_success(sc)      # over the scenarios that played
    assert mn == 0.5 and mean == pytest.approx((2 / 3 + 0.5) / 2)


def test_report_writes_the_scenario_csv(tmp_path):
    import torch
    res = torch.zeros((2, 4, 6), dtype=torch.float64)
    res[0, :, 0] = 1.0          # every first episode a success
    res[1, :, 1] = 1.0          # every second one a collision
    res[..., 3] = 5.0
    lines = []
    s = ev._report(res, 2, 4, 8, 1.0, 10, str(tmp_path), "m", lines.append, None, np.array([0, 1, 1, 0]), 2)
    assert s["episodes"] == 8 and [d["episodes"] for d in s["scenarios"]] == [4, 4]
    assert s["scenario_success_min"] == s["scenario_success_mean"] == 0.5
    txt = open(s["scenarios_csv"]).read().splitlines()
    assert s["scenarios_csv"].endswith("m_eval_scenarios.csv") and txt[0] == "scenario,episodes,success_rate,collision_rate,timeout_rate"
    assert txt[1:] == ["0,4,0.5,0.5,0.0", "1,4,0.5,0.5,0.0"]
    assert any("EVALUATION SCENARIOS" in ln and "min=50.00%" in ln for ln in lines)
    s0 = ev._report(res, 2, 4, 8, 1.0, 10, "", "m", None, None)    # without a bank: what it was
    assert "scenarios" not in s0


def test_abi_version_and_the_new_symbol():
    import ctypes
    from navbot_ppo_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    assert L.navsim_version() == 6 == _native.NAVSIM_ABI_VERSION
    assert hasattr(L, "navsim_set_mover_bank") and hasattr(L, "navsim_set_movers")
    res, args = {n: (r, a) for n, r, a in _native.SYMBOLS}["navsim_set_mover_bank"]
    assert res is ctypes.c_int and len(args) == 11
    fn = _native.lib().navsim_set_mover_bank
    assert fn(None, None, 0, 0, 0, None, None, None, None, 0, None) == -1 and b"navsim_set_mover_bank" in _native.lib().navsim_last_error()


def test_config_and_flags():
    from navbot_ppo_amd import main, ppo
    assert ppo.PPOConfig().eval_movers is None
    args = main.get_args(["--movers", "random:32", "--movers_seed", "4", "--eval_movers", "random:8", "--eval_every", "5"])
    assert main.movers_of(args.movers, args.movers_period, args.movers_seed) == dict(name="random:32", seed=4)
    cfg = main.config_of(args, 512)
    assert cfg.eval_movers == dict(name="random:8", seed=1)
    assert main.config_of(main.get_args([]), 512).eval_movers is None
    assert main.movers_of("bank:orbit4,patrol2", 16, 0) == dict(name="bank:orbit4,patrol2", period=16)
