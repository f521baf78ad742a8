"""Sector LiDAR (scan_pool) without a GPU: the host statement of the rule against the reference's own down-sampler, the selection
rule for pooled handles, and the refusals the Python layer makes before it looks for a device."""
import os
import subprocess

import numpy as np
import pytest

from navbot_ppo_amd import env as E
from navbot_ppo_amd import ppo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "navbot_ppo_amd", "csrc")


# ---------------------------------------------------------------- pool_scan_reference against the reference's Pick
@pytest.mark.parametrize("k", [2, 3, 4])
def test_pool_scan_reference_is_the_references_pick(k):
    """G11_pick.npz (tests/golden/generate_golden_pick.py): random and edge scans -- ties, 3.5, 0.12, -inf, +inf -- of 10 k samples
    and what the reference's pick_laser.Pick(scan, k) made of them"""
    g = np.load(os.path.join(HERE, "golden", "G11_pick.npz"))
    scan, want = g[f"scan_{k}"], g[f"pick_{k}"]
    assert scan.shape == (30, 10 * k) and want.shape == (30, 10)
    assert np.isneginf(scan).any() and np.isposinf(scan).any() and (scan == 3.5).any() and (scan == np.float32(0.12)).any()
    tail = np.arange(6, dtype=np.float32)[None].repeat(30, 0) + 100
    got = E.pool_scan_reference(np.concatenate([scan, tail], 1), k)
    assert got.shape == (30, 16) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:, :10].view(np.uint32), want.view(np.uint32))   # bit for bit, -inf included
    np.testing.assert_array_equal(got[:, 10:], tail)
    assert np.isneginf(want).sum() >= 3   # a -inf reading wins its column
    # leading axes pass through, k = 1 is the identity
    rows = np.concatenate([scan, tail], 1).reshape(5, 6, -1)
    np.testing.assert_array_equal(E.pool_scan_reference(rows, k), got.reshape(5, 6, 16))
    r16 = got.copy()
    np.testing.assert_array_equal(E.pool_scan_reference(r16, 1), r16)
    with pytest.raises(ValueError, match="columns"):
        E.pool_scan_reference(scan, k)


# ---------------------------------------------------------------- the selection rule
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sel") / "pool_dump"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "kernel_select_pool_dump.cpp"), "-o", str(exe)])
    return str(exe)


def test_scan_pool_1_picks_what_the_rule_picked(dump):
    got = subprocess.check_output([dump, "k1"], text=True).splitlines()
    want = open(os.path.join(HERE, "kernel_select_table.txt")).read().splitlines()
    assert got == want


ENTRIES = ("step", "step_seq", "rollout_mlp64", "rollout_hist", "rollout_resmlp512", "evaluate_mlp64", "evaluate_hist", "evaluate_resmlp512")


def test_pooled_picks(dump):
    rows = subprocess.check_output([dump, "pool"], text=True).splitlines()
    assert len(rows) == 3 * 12 * (8 * 2 * 2 * 6 + 3 * 2 * 6 + 11 * 2 * 6)   # k x envs x (10 beams shared +- movers, per-env; 36 beams)
    seen = set()
    for r in rows:
        facts, picks = r.split(" |")
        k, N, B, S, per_env, mov, sens, fe, boxes = (int(v) for v in facts.split())
        picks = [p.strip() for p in picks.split(";") if p.strip()]
        assert len(picks) == 8
        for name, p in zip(ENTRIES, picks):
            if B != 10:
                # (the history and 512-wide entries refuse 36 beams with their own, older sentence)
                assert p.startswith("-") and ("36-beam" in p and "not built" in p or name.endswith(("hist", "resmlp512"))), r
            elif per_env:
                assert p.startswith("-") and "per-env maps" in p and "not built" in p, r
            elif name.endswith("resmlp512"):
                assert p.startswith("-") and "512-wide" in p and "not built" in p, r
            else:   # the one pooled shape, whatever the shard size and navsim_set_shape say: the mover and sensor-options form
                assert p == f"0:16:8:{3 if boxes else 0}:1:1:{int(name.endswith('hist'))}:{k}", r
                seen.add((k, boxes, mov, N > 4096))
    assert seen == {(k, b, m, big) for k in (2, 3, 4) for b in (0, 1) for m in (0, 1) for big in (False, True)}


def test_pool_dump_under_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    exe = tmp_path / "pool_dump_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", CSRC, os.path.join(HERE, "kernel_select_pool_dump.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "pool"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]


# ---------------------------------------------------------------- refusals that need no device
@pytest.mark.parametrize("bad", [0, 5, -1, 2.0, "2", True, None])
def test_scan_pool_must_be_an_int_in_1_to_4(bad):
    for make in (lambda: E.NavSim(4, scan_pool=bad), lambda: E.VecEnv(4, scan_pool=bad), lambda: E.Env(True, scan_pool=bad),
                 lambda: E.check_scan_pool(bad)):
        with pytest.raises(ValueError, match="scan_pool"):
            make()


def test_scan_pool_refusals_name_what_is_not_built():
    with pytest.raises(ValueError, match="n_beams == 10.*not built"):
        E.NavSim(4, n_beams=36, scan_pool=2)
    with pytest.raises(ValueError, match="n_beams == 10.*not built"):
        E.VecEnv(4, n_beams=36, scan_pool=3)
    with pytest.raises(ValueError, match="per-env maps is not built"):
        E.VecEnv(4, per_env_map=True, scan_pool=2)
    with pytest.raises(ValueError, match="per-env maps is not built"):
        E.VecEnv(4, map=np.zeros((4, 8, 4), np.float32), scan_pool=2)
    with pytest.raises(ValueError, match="resmlp512.*not built"):
        E.check_scan_pool(2, policy="resmlp512")
    assert E.check_scan_pool(4, 10, False, "mlp64x2") == 4 and E.check_scan_pool(1, 36, True, "resmlp512") == 1


def test_trainer_refuses_the_wide_nets_on_a_pooled_env():
    class Sim:
        scan_pool = 2

    class FakeEnv:
        N, B, D, sim = 4, 10, 16, Sim()
        import torch
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="resmlp512.*not built"):
        ppo.PPOTrainer(FakeEnv(), ppo.PPOConfig(rollout_len=4, policy="resmlp512"))


def test_main_takes_scan_pool():
    from navbot_ppo_amd import main
    assert main.get_args([]).scan_pool == 1 and main.get_args(["--scan_pool", "4"]).scan_pool == 4
    with pytest.raises(SystemExit):
        main.get_args(["--scan_pool", "5"])


def test_log_keys_only_when_pooled():
    from navbot_ppo_amd import train_log
    lg = dict(iteration=1, t_so_far=10, avg_ep_rews=0.0, success_rate=0.0, avg_ep_lens=1.0, actor_loss=0.0, critic_loss=0.0,
              approx_kl=0.0, steps_per_sec=1.0, rollout_time=0.1, update_time=0.1)
    cfg = ppo.PPOConfig()
    assert "scan_pool" not in train_log.progress_line(lg) and "env/scan_pool" not in train_log.tb_scalars(lg, cfg)
    lg["scan_pool"] = 4
    assert " scan_pool=4" in train_log.progress_line(lg) and train_log.tb_scalars(lg, cfg)["env/scan_pool"] == 4
