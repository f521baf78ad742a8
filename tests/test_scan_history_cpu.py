"""Scan history (PPOConfig.scan_history, navsim_stack_rows, navsim_rollout_mlp64_hist, navsim_evaluate_mlp64_hist) as far as it can
be checked without a device: the host statement of the row rule on hand-made rows, the window property a stepping loop relies on,
the single-env deque, the configuration surface with every refusal that needs no GPU, and the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from navbot_ppo_amd import _native, env as envmod, evaluate as ev, main, nets, ppo
from navbot_ppo_amd.env import HIST_DIM, HostHistoryWindow, stack_rows_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(R, N, dtype=np.float32, seed=0):
    """distinct values everywhere: entry (t, n, c) = (64 t + 16 n + c) / 1024, exact in float16 for R <= 8, N <= 4"""
    assert R <= 8 and N <= 4
    t, n, c = np.meshgrid(np.arange(R), np.arange(N), np.arange(16), indexing="ij")
    return ((64 * t + 16 * n + c) / 1024.0).astype(dtype)


def expect_row(obs, t, n, i1, i2):
    out = np.zeros(HIST_DIM, dtype=obs.dtype)
    out[0:16] = obs[t, n]
    out[16:26] = obs[i1, n, 0:10]
    out[26:36] = obs[i2, n, 0:10]
    out[36:38] = obs[i1, n, 10:12]
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_rule_on_hand_made_rows(dtype):
    R, N = 7, 4
    obs = rows(R, N, dtype)
    ended = np.zeros((R - 1, N), dtype=np.uint8)
    # env 0: no cut but row 0.  env 1: cuts on two consecutive rows (rows 2 and 3 start episodes).  env 2: a cut on the last row.
    # env 3: a cut on row 1 and one two rows later (less than three rows apart).
    ended[1, 1] = ended[2, 1] = 1
    ended[R - 2, 2] = 1
    ended[0, 3] = ended[2, 3] = 1
    out = stack_rows_reference(obs, ended)
    assert out.shape == (R, N, HIST_DIM) and out.dtype == obs.dtype
    want = {   # per env: (i1, i2) of every row
        0: [(0, 0), (0, 0), (1, 0), (2, 1), (3, 2), (4, 3), (5, 4)],
        1: [(0, 0), (0, 0), (2, 2), (3, 3), (3, 3), (4, 3), (5, 4)],
        2: [(0, 0), (0, 0), (1, 0), (2, 1), (3, 2), (4, 3), (6, 6)],
        3: [(0, 0), (1, 1), (1, 1), (3, 3), (3, 3), (4, 3), (5, 4)],
    }
    for n, pairs in want.items():
        for t, (i1, i2) in enumerate(pairs):
            assert np.array_equal(out[t, n], expect_row(obs, t, n, i1, i2)), (n, t)
    assert not out[:, :, 38:].any()
    # an episode's first row: all three frames are its own scan, columns 36..37 its own past_action
    assert np.array_equal(out[3, 1, 16:26], obs[3, 1, 0:10]) and np.array_equal(out[3, 1, 26:36], obs[3, 1, 0:10])
    assert np.array_equal(out[3, 1, 36:38], obs[3, 1, 10:12])


@pytest.mark.parametrize("R", [1, 2, 3])
def test_short_buffers(R):
    obs = rows(R, 3)
    ended = None if R == 1 else np.zeros((R - 1, 3), dtype=np.uint8)
    out = stack_rows_reference(obs, ended)
    for t in range(R):
        for n in range(3):
            assert np.array_equal(out[t, n], expect_row(obs, t, n, max(t - 1, 0), max(t - 2, 0)))
    if R > 1:
        with pytest.raises(ValueError):
            stack_rows_reference(obs, None)
    with pytest.raises(ValueError):
        stack_rows_reference(obs[:, :, :15], ended)


def test_every_cut_pattern_of_three_rows_and_the_window_property():
    """out[-1] of the rows t-2..t equals row t of the full stack, whatever lies in front of the window"""
    rng = np.random.default_rng(5)
    R, N = 40, 64
    obs = rng.standard_normal((R, N, 16)).astype(np.float32)
    ended = (rng.random((R - 1, N)) < 0.3).astype(np.uint8)
    full = stack_rows_reference(obs, ended)
    for t in range(R):
        lo = max(t - 2, 0)
        win = stack_rows_reference(obs[lo:t + 1], ended[lo:t] if t > lo else None)
        assert np.array_equal(win[-1], full[t]), t
    # densities 0 and 1
    none, every = stack_rows_reference(obs, np.zeros_like(ended)), stack_rows_reference(obs, np.ones_like(ended))
    assert np.array_equal(every[:, :, 16:26], obs[:, :, 0:10]) and np.array_equal(every[:, :, 26:36], obs[:, :, 0:10])
    assert np.array_equal(every[:, :, 36:38], obs[:, :, 10:12])
    assert np.array_equal(none[2:, :, 16:26], obs[1:-1, :, 0:10]) and np.array_equal(none[2:, :, 26:36], obs[:-2, :, 0:10])
    assert np.array_equal(none[1, :, 26:36], obs[0, :, 0:10]) and np.array_equal(none[1:, :, 36:38], obs[:-1, :, 10:12])


def test_host_window_is_the_reference():
    """the three-row deque of Env(scan_history=True) against the full stack, with resets in between"""
    rng = np.random.default_rng(9)
    R = 30
    obs = rng.standard_normal((R, 1, 16)).astype(np.float32)
    ended = (rng.random((R - 1, 1)) < 0.25).astype(np.uint8)
    full = stack_rows_reference(obs, ended)
    w = HostHistoryWindow()
    with pytest.raises(ValueError):
        w.push(obs[0, 0], 0)
    got = [w.reset(obs[0, 0])]
    for t in range(1, R):
        got.append(w.push(obs[t, 0], ended[t - 1, 0]))
    assert np.array_equal(np.stack(got), full[:, 0])
    assert got[0].shape == (HIST_DIM,) and got[0].dtype == np.float32
    # a reset() in the middle is an episode start whatever the flag said
    r = w.reset(obs[7, 0])
    assert np.array_equal(r, expect_row(obs, 7, 0, 7, 7))


def test_config_validation_and_flags():
    assert ppo.PPOConfig().scan_history is False
    cfg = ppo.PPOConfig(policy="mlp64x2", scan_history=True)
    assert cfg.scan_history is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="scan_history"):
            ppo.PPOConfig(policy="mlp64x2", scan_history=bad)
    with pytest.raises(ValueError, match="16-column"):
        ppo.PPOConfig(policy="resmlp512", scan_history=True)
    with pytest.raises(ValueError, match="persistent_rollout"):
        ppo.PPOConfig(policy="mlp64x2", scan_history=True, persistent_rollout=False)
    with pytest.raises(ValueError, match="fused_update"):
        ppo.PPOConfig(policy="mlp64x2", scan_history=True, fused_update=False)
    ok = ppo.PPOConfig(policy="mlp64x2")
    ok.scan_history = "on"   # a config is mutable: the check runs again where the option is put to use
    with pytest.raises(ValueError, match="scan_history"):
        ppo.check_scan_history_config(ok)
    a = main.get_args(["--scan_history", "--policy", "mlp64x2"])
    assert a.scan_history is True and main.config_of(a, 8).scan_history is True
    a = main.get_args([])
    assert a.scan_history is False and main.config_of(a, 8).scan_history is False


class _FakeSim:
    obs_dtype = torch.float32


class _FakeEnv:
    """what PPOTrainer reads of an env before it touches a device"""
    def __init__(self, B, device):
        self.N, self.B, self.D, self.device, self.sim = 4, B, B + 6, torch.device(device), _FakeSim()


def test_trainer_refusals_without_a_device():
    cfg = ppo.PPOConfig(policy="mlp64x2", scan_history=True, rollout_len=4)
    with pytest.raises(ValueError, match="n_beams == 10"):
        ppo.PPOTrainer(_FakeEnv(36, "cpu"), cfg)
    with pytest.raises(ValueError, match="GPU"):
        ppo.PPOTrainer(_FakeEnv(10, "cpu"), cfg)
    cfg2 = ppo.PPOConfig(policy="mlp64x2", rollout_len=4)
    cfg2.policy = "resmlp512"
    cfg2.scan_history = True
    with pytest.raises(ValueError, match="16-column"):
        ppo.PPOTrainer(_FakeEnv(10, "cpu"), cfg2)


def test_policy_sizes_and_checkpoint_detection():
    a, c = nets.make_policy("mlp64x2", HIST_DIM)
    assert sum(p.numel() for p in a.parameters()) == 7042 and sum(p.numel() for p in c.parameters()) == 6977
    assert nets.flat_actor_params(a).numel() == 7042
    assert ev.reads_scan_history(a) and not ev.reads_scan_history(a, n_beams=36)
    a16, _ = nets.make_policy("mlp64x2", 16)
    assert not ev.reads_scan_history(a16) and not ev.reads_scan_history(torch.nn.Linear(42, 2))
    assert ev.persistent_policy(a)[0] == "mlp64x2" and ev.persistent_policy(a)[1].numel() == 7042


def test_no_cpu_path():
    with pytest.raises(_native.NavsimError):
        envmod.stack_rows(torch.zeros((2, 3, 16)), torch.zeros((1, 3), dtype=torch.uint8))


def test_exports_and_bindings():
    for name in ("stack_rows", "stack_rows_reference", "HistoryWindow", "HostHistoryWindow"):
        assert name in envmod.__all__ and hasattr(envmod, name)
    bound = {n: (r, a) for n, r, a in _native.SYMBOLS}
    for name in ("navsim_stack_rows", "navsim_rollout_mlp64_hist", "navsim_evaluate_mlp64_hist"):
        assert name in bound
    assert len(bound["navsim_rollout_mlp64_hist"][1]) == len(bound["navsim_rollout_mlp64"][1])
    assert len(bound["navsim_evaluate_mlp64_hist"][1]) == len(bound["navsim_evaluate_mlp64"][1])
    assert _native.NAVSIM_ABI_VERSION == 6   # additions only
    # the header declares them with as many parameters as the table binds
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "navsim.h")).read(), flags=re.S)
    for name in ("navsim_stack_rows", "navsim_rollout_mlp64_hist", "navsim_evaluate_mlp64_hist"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name][1]), name
    L = _native.lib()
    assert hasattr(L, "navsim_stack_rows")


def test_argument_checks_run_before_any_device_call():
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # (never dereferenced: every call below is refused first)
    assert L.navsim_stack_rows(None, 0, None, 1, 1, p, None) == -1
    assert L.navsim_stack_rows(p, 0, None, 1, 1, None, None) == -1
    assert L.navsim_stack_rows(p, 0, None, 0, 1, p, None) == -1 and b"at least 1" in L.navsim_last_error()
    assert L.navsim_stack_rows(p, 0, None, 1, 0, p, None) == -1
    assert L.navsim_stack_rows(p, 0, None, 2, 1, p, None) == -1 and b"ended_dev" in L.navsim_last_error()
    assert L.navsim_stack_rows(ctypes.c_void_p(p.value + 4), 0, None, 1, 1, p, None) == -1 and b"aligned" in L.navsim_last_error()
    assert L.navsim_stack_rows(p, 0, None, 1, 1, ctypes.c_void_p(p.value + 8), None) == -1
    for name in ("navsim_rollout_mlp64_hist",):
        assert getattr(L, name)(*([None] * 13), 0, None, 1, None) == -1
    assert L.navsim_evaluate_mlp64_hist(None, None, None, 1, 1, None, None, None, None, None, None, None) == -1
    assert b"navsim_evaluate_mlp64_hist" in L.navsim_last_error()
