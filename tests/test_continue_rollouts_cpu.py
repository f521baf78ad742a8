"""Rollouts that continue across iterations (PPOConfig.continue_rollouts, navsim_rollout_mlp64_hist_cont, navsim_stack_rows_cont) as
far as they can be checked without a device: the host mirrors chained through their carries against the uncut buffer, every refusal
of the configuration, the trainer state with the option off and on, and the bindings."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from navbot_ppo_amd import _native, env as envmod, main, ppo
from navbot_ppo_amd.env import HIST_CARRY, HIST_DIM, stack_rows_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N = 12, 24


def _buffer(dtype=np.float32, seed=3):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((R, N, 16)).astype(dtype)
    ended = (rng.random((R - 1, N)) < 0.3).astype(np.uint8)
    return obs, ended


def _chain(obs, ended, cuts):
    """the pieces obs[a : b + 1] between consecutive cut rows, each continued from the carry of the one before"""
    edges = [0] + list(cuts) + [obs.shape[0] - 1]
    rows, carry, last = [], None, None
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        piece, flags = obs[a:b + 1], (ended[a:b] if b > a else None)
        if carry is None:   # the first piece starts the episodes; its carry-out is columns 16..37 of its last row
            out = stack_rows_reference(piece, flags)
            carry = out[-1, :, 16:38].astype(np.float32)
        else:
            out, carry = stack_rows_reference(piece, flags, carry=carry)
        rows.append(out if k == 0 else out[1:])   # a piece's row 0 is the row the piece before ended on
        assert k == 0 or np.array_equal(out[0], last), ("seam row", a)
        last = out[-1]
    return np.concatenate(rows), carry


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_stack_rows_reference_chained_equals_the_whole(dtype):
    obs, ended = _buffer(dtype)
    assert 0.2 < ended.mean() < 0.4
    full = stack_rows_reference(obs, ended)
    for s in range(1, R):   # every cut point (at R - 1 the second piece is the last row alone: its history row is the carry)
        got, carry = _chain(obs, ended, [s])
        assert got.dtype == obs.dtype and np.array_equal(got, full), s
        assert carry.dtype == np.float32 and carry.shape == (N, HIST_CARRY)
        assert np.array_equal(carry, full[-1, :, 16:38].astype(np.float32)), s
    # three pieces with a middle piece of ONE step (two rows: the seam rows themselves), at every position
    for s in range(1, R - 2):
        got, _ = _chain(obs, ended, [s, s + 1])
        assert np.array_equal(got, full), s
    # a middle piece of one ROW (R == 1: no flags at all): it hands its carry on unchanged
    out, c1 = stack_rows_reference(obs[:5], ended[:4], carry=np.zeros((N, HIST_CARRY), np.float32))
    one, c2 = stack_rows_reference(obs[4:5], None, carry=c1)
    assert np.array_equal(one[0], out[-1]) and np.array_equal(c1, c2)


def test_stack_rows_reference_carry_surface():
    obs, ended = _buffer()
    assert isinstance(stack_rows_reference(obs, ended), np.ndarray)   # without a carry: the rows alone, as before
    with pytest.raises(ValueError, match="carry"):
        stack_rows_reference(obs, ended, carry=np.zeros((N, 21), np.float32))
    # the carry IS columns 16..37 of row 0, and row 1 reads its oldest frame from it unless the step between ended the episode
    carry = np.random.default_rng(1).standard_normal((N, HIST_CARRY)).astype(np.float32)
    out, _ = stack_rows_reference(obs, ended, carry=carry)
    assert np.array_equal(out[0, :, 16:38], carry) and np.array_equal(out[0, :, :16], obs[0]) and not out[:, :, 38:].any()
    keep = ended[0] == 0
    assert keep.any() and (~keep).any()
    assert np.array_equal(out[1, keep, 26:36], carry[keep, 0:10]) and np.array_equal(out[1, keep, 16:26], obs[0, keep, 0:10])
    assert np.array_equal(out[1, ~keep, 26:36], obs[1, ~keep, 0:10])
    assert np.array_equal(out[2:], stack_rows_reference(obs, ended)[2:])   # from row 2 on nothing looks in front of row 0


def test_reward_norm_reference_chained_through_its_carry():
    rng = np.random.default_rng(11)
    T = 16
    rew = rng.standard_normal((T, N)).astype(np.float32) * 30
    ended = (rng.random((T, N)) < 0.3).astype(np.uint8)
    whole = ppo.reward_norm_reference(rew, ended, 0.99)
    # the running returns of the whole, for the moments of the pieces
    for cuts in [[s] for s in range(1, T)] + [[5, 6]]:
        edges = [0] + cuts + [T]
        carry, n, rets_sum, rets_sq = None, 0, 0.0, 0.0
        for a, b in zip(edges[:-1], edges[1:]):
            r = ppo.reward_norm_reference(rew[a:b], ended[a:b], 0.99, carry=carry)
            carry = r.carry
            cnt, mean, m2 = r.moments
            n += cnt
            rets_sum += cnt * mean
            rets_sq += m2 + cnt * mean * mean
        assert np.array_equal(carry, whole.carry), cuts   # the running return behind the last row: the same float64 chain
        mean = rets_sum / n
        np.testing.assert_allclose([n, mean, rets_sq - n * mean * mean], whole.moments, rtol=1e-9)
    # without the carry the second piece starts its columns at 0: another running return wherever an episode runs across the cut
    assert not np.array_equal(ppo.reward_norm_reference(rew[8:], ended[8:], 0.99).moments,
                              ppo.reward_norm_reference(rew[8:], ended[8:], 0.99, carry=ppo.reward_norm_reference(rew[:8], ended[:8], 0.99).carry).moments)


def test_config_refusals_and_flags():
    assert ppo.PPOConfig().continue_rollouts is False
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="continue_rollouts"):
            ppo.PPOConfig(continue_rollouts=bad, bootstrap_truncated=True)
    # the batch end must not be terminal
    with pytest.raises(ValueError, match="batch end"):
        ppo.PPOConfig(continue_rollouts=True)
    with pytest.raises(ValueError, match="batch end"):
        ppo.PPOConfig(continue_rollouts=True, gae_lambda=1.0)
    assert ppo.PPOConfig(continue_rollouts=True, bootstrap_truncated=True).continue_rollouts is True
    assert ppo.PPOConfig(continue_rollouts=True, gae_lambda=0.95).continue_rollouts is True
    assert ppo.PPOConfig(continue_rollouts=True, gae_lambda=1.0, bootstrap_truncated=True).continue_rollouts is True
    ok = ppo.PPOConfig(continue_rollouts=True, bootstrap_truncated=True)
    ok.bootstrap_truncated = False   # a config is mutable: the check runs again where the option is put to use
    with pytest.raises(ValueError, match="batch end"):
        ppo.check_continue_config(ok)
    with pytest.raises(ValueError, match="batch end"):
        ppo.PPOTrainer(_FakeEnv(), ok)
    a = main.get_args(["--continue_rollouts", "--bootstrap_truncated"])
    assert a.continue_rollouts is True and main.config_of(a, 8).continue_rollouts is True
    a = main.get_args([])
    assert a.continue_rollouts is False and main.config_of(a, 8).continue_rollouts is False


class _FakeSim:
    obs_dtype = torch.float32
    cfg = types.SimpleNamespace(env_id_base=0)
    generation = 0

    def __init__(self):
        self.resets = 0

    def reset(self, obs):
        self.resets += 1
        obs.fill_(float(self.resets))


class _FakeEnv:
    """what PPOTrainer reads of an env before it touches a device"""
    def __init__(self):
        self.N, self.B, self.D, self.device, self.sim = 4, 10, 16, torch.device("cpu"), _FakeSim()


def _tensors(t):
    return {k: (tuple(v.shape), v.dtype) for k, v in vars(t).items() if torch.is_tensor(v)}


def test_option_off_builds_the_trainer_state_it_built_before():
    base = dict(policy="mlp64x2", rollout_len=4, norm_reward=True, bootstrap_truncated=True)
    off = ppo.PPOTrainer(_FakeEnv(), ppo.PPOConfig(**base))
    assert off.continue_rollouts is False
    # the tensors of a trainer with the option off: the list as it stood before the option existed
    assert set(_tensors(off)) == {"obs_buf", "act_buf", "logp_buf", "rew_buf", "done_buf", "arrive_buf", "ended_buf", "epret_buf",
                                  "eplen_buf", "eppath_buf", "rtg_buf", "ret_rms", "rew_scaled_buf", "_ret_rows", "var", "_lo", "_hi",
                                  "_step_base"}
    assert not hasattr(off, "_hist_carry") and not hasattr(off, "_ret_carry")
    on = ppo.PPOTrainer(_FakeEnv(), ppo.PPOConfig(continue_rollouts=True, **base))
    extra = {k: v for k, v in _tensors(on).items() if k not in _tensors(off)}
    assert extra == {"_ret_carry": ((4,), torch.float64)} and not on._ret_carry.any()
    assert {k: v for k, v in _tensors(on).items() if k in _tensors(off)} == _tensors(off)


def test_when_row_zero_is_a_reset_row():
    """_begin_rollout: off -- every rollout resets; on -- the first one, one behind reset_envs() / a changed world, and otherwise row T
    of the last batch becomes row 0"""
    base = dict(policy="mlp64x2", rollout_len=4, norm_reward=True, bootstrap_truncated=True)
    off = ppo.PPOTrainer(_FakeEnv(), ppo.PPOConfig(**base))
    for k in range(3):
        off._begin_rollout()
        assert off._did_reset and off.env.sim.resets == k + 1
    on = ppo.PPOTrainer(_FakeEnv(), ppo.PPOConfig(continue_rollouts=True, **base))
    sim = on.env.sim
    on._begin_rollout()
    assert on._did_reset and sim.resets == 1
    on.obs_buf[4].fill_(7.0)
    on._ret_carry.fill_(3.0)
    on._begin_rollout()
    assert not on._did_reset and sim.resets == 1 and (on.obs_buf[0] == 7.0).all() and (on._ret_carry == 3.0).all()
    on.reset_envs()
    on._begin_rollout()
    assert on._did_reset and sim.resets == 2 and (on.obs_buf[0] == 2.0).all() and not on._ret_carry.any()
    on._begin_rollout()
    assert not on._did_reset and sim.resets == 2
    sim.generation = 5   # set_map / set_movers / the spawn sampler
    on._begin_rollout()
    assert on._did_reset and sim.resets == 3
    on._begin_rollout()
    assert not on._did_reset
    on._begin_rollout(capturing=True)   # a graph capture warms up by stepping the envs: such a rollout resets
    assert on._did_reset and sim.resets == 4
    # exploration decay: the N episode starts of a reset are counted for rollouts that did reset only
    on._did_reset = False
    on._rollout_metrics([8.0, 1, 1, 6, 40.0, 3.0])
    assert on.episode_starts == 8.0
    on._did_reset = True
    on._rollout_metrics([8.0, 1, 1, 6, 40.0, 3.0])
    assert on.episode_starts == 8.0 + on.env.N


def test_bindings_and_header():
    for name in ("HIST_CARRY",):
        assert name in envmod.__all__
    assert HIST_CARRY == 22 and HIST_DIM == 42
    bound = {n: (r, a) for n, r, a in _native.SYMBOLS}
    assert len(bound["navsim_rollout_mlp64_hist_cont"][1]) == len(bound["navsim_rollout_mlp64_hist"][1]) + 2
    assert len(bound["navsim_stack_rows_cont"][1]) == len(bound["navsim_stack_rows"][1]) + 2
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "navsim.h")).read(), flags=re.S)
    for name in ("navsim_rollout_mlp64_hist_cont", "navsim_stack_rows_cont"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(bound[name][1]), name
    assert "loses two frames" not in open(os.path.join(REPO, "include", "navsim.h")).read()


def test_argument_checks_run_before_any_device_call():
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # (never dereferenced: every call below is refused first)
    off = ctypes.c_void_p(p.value + 8)
    # what navsim_stack_rows refuses
    assert L.navsim_stack_rows_cont(None, 0, None, 1, 1, p, None, None, None) == -1
    assert L.navsim_stack_rows_cont(p, 0, None, 0, 1, p, None, None, None) == -1 and b"at least 1" in L.navsim_last_error()
    assert L.navsim_stack_rows_cont(p, 0, None, 2, 1, p, None, None, None) == -1 and b"ended_dev" in L.navsim_last_error()
    assert L.navsim_stack_rows_cont(off, 0, None, 1, 1, p, None, None, None) == -1
    # ... and a misaligned carry, either one
    assert L.navsim_stack_rows_cont(p, 0, None, 1, 1, p, off, None, None) == -1 and b"carries" in L.navsim_last_error()
    assert L.navsim_stack_rows_cont(p, 0, None, 1, 1, p, None, off, None) == -1 and b"carries" in L.navsim_last_error()
    assert L.navsim_rollout_mlp64_hist_cont(*([None] * 13), 0, None, 1, None, None, None) == -1
    assert b"navsim_rollout_mlp64_hist_cont" in L.navsim_last_error()
    with pytest.raises(_native.NavsimError):
        envmod.stack_rows(torch.zeros((2, 3, 16)), torch.zeros((1, 3), dtype=torch.uint8), carry_in=torch.zeros((3, 22)))
