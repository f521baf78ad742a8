"""PPOConfig.norm_reward without a GPU: the host mirror (ppo.reward_norm_reference) against a per-step loop that restates what
Stable-Baselines3's VecNormalize.step / RunningMeanStd.update do (Stable-Baselines3 itself is not a dependency: parity is pinned to this
literal restatement of its published code, not to the package), the configuration's validation, the argument refusals of the two C entry
points (they come before any HIP call), the command-line flags and the third checkpoint file."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from navbot_ppo_amd import main as cli
from navbot_ppo_amd import nets, ppo
from navbot_ppo_amd._native import NavsimError, lib

from _rewards import synthetic_rollout

GAMMA = 0.99


class RunningMeanStd:
    """stable_baselines3.common.running_mean_std.RunningMeanStd for a scalar, restated"""

    def __init__(self, epsilon=1e-4):
        self.mean, self.var, self.count = np.float64(0.0), np.float64(1.0), epsilon

    def update(self, arr):
        self.update_from_moments(np.mean(arr, axis=0), np.var(arr, axis=0), arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / tot_count
        self.mean, self.var, self.count = new_mean, m_2 / tot_count, batch_count + self.count


def vecnormalize_loop(rew, ended, gamma):
    """VecNormalize.step's return bookkeeping, per step: ret = ret * gamma + r; ret_rms.update(ret); ret[done] = 0"""
    rms = RunningMeanStd()
    ret = np.zeros(rew.shape[1])
    for t in range(rew.shape[0]):
        ret = ret * gamma + rew[t]
        rms.update(ret)
        ret[ended[t] != 0] = 0
    return rms


@pytest.mark.parametrize("T,N", [(1, 1), (33, 5), (97, 37), (512, 4096)])
def test_mirror_has_the_final_statistics_of_a_per_step_loop(T, N):
    rew, ended = synthetic_rollout(T, N)
    if (T, N) == (1, 1):
        rew[0, 0] = 7.0   # the prior-dominated case: one return against a prior of count 1e-4 and variance 1
    want = vecnormalize_loop(rew, ended, GAMMA)
    got = ppo.reward_norm_reference(rew, ended, GAMMA)
    mean, var, count, scale = got.rms
    print(f"T={T} N={N}: dmean/std {abs(mean - want.mean) / np.sqrt(want.var):.3g}  dvar/var {abs(var - want.var) / want.var:.3g}  "
          f"count {count!r} vs {want.count!r}")
    assert abs(mean - want.mean) <= 1e-12 * np.sqrt(want.var)
    assert abs(var - want.var) <= 1e-12 * want.var
    assert count == want.count
    assert scale == 1.0 / np.sqrt(var + 1e-8)
    assert got.moments[0] == T * N and got.out.dtype == np.float32 and got.out.shape == (T, N)
    np.testing.assert_array_equal(got.out, np.clip((rew.astype(np.float64) * scale).astype(np.float32), -10.0, 10.0))
    if (T, N) == (1, 1):
        assert 13.0 < scale < 15.0 and got.out[0, 0] == 10.0   # 7 x 14.1 = 99: the clip is active
    else:
        assert np.abs(got.out).max() <= 10.0 and (np.abs(got.out) < 10.0).any()


def test_mirror_carry_and_split_rollouts():
    """the mirror over rows 0..48 and then, with the carry, over 49..96, merged row by row: the one call's statistics and carry"""
    rew, ended = synthetic_rollout(97, 37, seed=3, p_end=0.03)
    whole = ppo.reward_norm_reference(rew, ended, GAMMA)
    a = ppo.reward_norm_reference(rew[:49], ended[:49], GAMMA)
    b = ppo.reward_norm_reference(rew[49:], ended[49:], GAMMA, carry=a.carry)
    np.testing.assert_array_equal(b.carry, whole.carry)
    assert (whole.carry[ended[-1] != 0] == 0).all()
    m = ppo.merge_return_moments(ppo.RET_RMS_INIT, [a.moments, b.moments])
    assert abs(m[0] - whole.rms[0]) <= 1e-12 * np.sqrt(whole.rms[1]) and abs(m[1] - whole.rms[1]) <= 1e-12 * whole.rms[1]
    assert m[2] == whole.rms[2]
    # a row without samples and a poisoned row leave the statistics alone, bit for bit
    bad = [[0.0, 5.0, 5.0], [10.0, np.nan, 1.0], [10.0, 1.0, np.inf]]
    np.testing.assert_array_equal(ppo.merge_return_moments(m, bad), m)


# ------------------------------------------------------------------------------------------------ configuration and flags
def test_config_defaults_and_validation():
    cfg = ppo.PPOConfig()
    assert cfg.norm_reward is False and cfg.clip_reward == 10.0 and cfg.norm_reward_eps == 1e-8
    assert ppo.PPOConfig(norm_reward=True, clip_reward=5, norm_reward_eps=0.0).clip_reward == 5
    for bad in (0.0, -1.0, float("nan"), None, True):
        with pytest.raises(ValueError):
            ppo.PPOConfig(clip_reward=bad)
    for bad in (-1e-12, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError):
            ppo.PPOConfig(norm_reward_eps=bad)


def test_cli_flags_reach_the_config():
    cfg = cli.config_of(cli.get_args(["--norm_reward", "--clip_reward", "5"]), 8)
    assert cfg.norm_reward is True and cfg.clip_reward == 5.0
    cfg = cli.config_of(cli.get_args([]), 8)
    assert cfg.norm_reward is False and cfg.clip_reward == 10.0


def test_no_cpu_path():
    rew, ended = (torch.from_numpy(a) for a in synthetic_rollout(4, 4))
    with pytest.raises(NavsimError):
        ppo.return_moments(rew, ended, GAMMA)
    with pytest.raises(NavsimError):
        ppo.reward_scale(torch.tensor([0.0, 1.0, 1e-4, 1.0], dtype=torch.float64), None, rew)


# ------------------------------------------------------------------------------------------------ refusals of the C entry points
P = 0x10000   # a non-null, 256-byte aligned address that is never dereferenced: every call below is refused before any HIP call


def _refused(rc, who):
    msg = lib().navppo_last_error().decode()
    assert rc != 0 and msg.startswith(who + ":"), (rc, msg)


def test_return_moments_refuses_bad_arguments_without_a_device():
    f = lib().navppo_return_moments
    who = "navppo_return_moments"
    good = dict(rew=P, ended=P, T=8, N=16, gamma=0.99, carry=P, moments=P)
    bad = [dict(rew=None), dict(ended=None), dict(moments=None), dict(T=0), dict(T=-1), dict(N=0), dict(N=-16), dict(gamma=-0.01),
           dict(gamma=1.0000001), dict(gamma=float("nan")), dict(moments=P + 4), dict(carry=P + 4), dict(rew=P + 2)]
    for change in bad:
        a = dict(good, **change)
        _refused(f(a["rew"], a["ended"], a["T"], a["N"], a["gamma"], a["carry"], a["moments"], None), who)


def test_reward_scale_refuses_bad_arguments_without_a_device():
    f = lib().navppo_reward_scale
    who = "navppo_reward_scale"
    good = dict(rms=P, moments=P, K=1, rin=P, rout=P, n=64, eps=1e-8, clip=10.0)
    bad = [dict(rms=None), dict(moments=None), dict(rin=None), dict(rout=None), dict(K=-1), dict(n=-1), dict(eps=-1e-9),
           dict(eps=float("nan")), dict(clip=0.0), dict(clip=-10.0), dict(clip=float("nan")), dict(rms=P + 4), dict(moments=P + 4),
           dict(rin=P + 1), dict(rout=P + 2)]
    for change in bad:
        a = dict(good, **change)
        _refused(f(a["rms"], a["moments"], a["K"], a["rin"], a["rout"], C.c_int64(a["n"]), a["eps"], a["clip"], None), who)


# ------------------------------------------------------------------------------------------------ the third checkpoint file
def _bare_trainer(tmp_path, **cfg):
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg = ppo.PPOConfig(output_dir=str(tmp_path), method_name="m", policy="mlp64x2", **cfg)
    t.actor, t.critic = nets.make_policy("mlp64x2")
    t.i_so_far, t.t_so_far = 4, 19876
    if t.cfg.norm_reward:
        t._init_ret_rms("cpu")
    return t


def test_checkpoint_roundtrip_of_the_return_statistics(tmp_path):
    t = _bare_trainer(tmp_path, norm_reward=True)
    assert t.ret_rms.tolist()[:3] == [0.0, 1.0, 1e-4] and t.ret_rms.dtype == torch.float64
    t._init_ret_rms("cpu", 12.5, 3456.789, 2097152.0001)
    pa, pc = t.save_checkpoint()
    d = os.path.dirname(pa)
    assert sorted(os.listdir(d)) == ["actor_iter0004_step00019876.pth", "critic_iter0004_step00019876.pth", "retnorm_iter0004_step00019876.pth"]
    assert torch.load(os.path.join(d, "retnorm_iter0004_step00019876.pth")) == {"mean": 12.5, "var": 3456.789, "count": 2097152.0001}
    t2 = _bare_trainer(tmp_path, norm_reward=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t2.load_checkpoint(pa, pc)
    assert torch.equal(t2.ret_rms, t.ret_rms) and t2.ret_rms[3] == 1.0 / np.sqrt(3456.789 + 1e-8)
    for k, v in t.actor.state_dict().items():
        assert torch.equal(v, t2.actor.state_dict()[k])


def test_a_missing_statistics_file_warns_and_starts_fresh(tmp_path):
    off = _bare_trainer(tmp_path)   # the option off: two files, as before
    pa, pc = off.save_checkpoint()
    assert len(os.listdir(os.path.dirname(pa))) == 2 and not hasattr(off, "ret_rms")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off.load_checkpoint(pa, pc)
    on = _bare_trainer(tmp_path, norm_reward=True)
    on._init_ret_rms("cpu", 1.0, 2.0, 3.0)
    with pytest.warns(UserWarning, match="retnorm_iter0004_step00019876.pth not found") as rec:
        on.load_checkpoint(pa, pc)
    assert len(rec) == 1 and "\n" not in str(rec[0].message)
    assert on.ret_rms.tolist()[:3] == [0.0, 1.0, 1e-4]
