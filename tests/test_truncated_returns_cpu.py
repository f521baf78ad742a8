"""PPOConfig.bootstrap_truncated without a GPU: the host mirror (env.truncated_returns_reference) against a literal restatement of
rsl_rl's RolloutStorage.compute_returns with its `rewards += gamma * values * time_outs` in front (rsl_rl itself is not a dependency:
parity is pinned to this restatement of its published rule, not to the package), the reductions of the mirror, the argument refusals
of navsim_gae_scan_trunc (they come before any HIP call), the configuration's validation and the command-line flag."""
import numpy as np
import pytest

from navbot_ppo_amd import main as cli
from navbot_ppo_amd import ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import truncated_returns_reference

from _truncation import truncated_batch, truncated_rows

GAMMA = 0.99
SHAPES = [(1, 16), (33, 16), (545, 48)]
LAMBDAS = [0.0, 0.95, 1.0]


def rsl_rl_returns(rew, ended, time_outs, values, last_values, gamma, lam):
    """rsl_rl, restated in float64: the environment step's `rewards += gamma * values * time_outs` (the values are those of the
    observation the action was chosen from), then RolloutStorage.compute_returns: delta = r + not_terminal gamma V' - V,
    advantage = delta + not_terminal gamma lam advantage', returns = advantage + V, with `dones` = every episode end."""
    T, N = rew.shape
    values = values.astype(np.float64)
    rewards = rew.astype(np.float64) + gamma * values * time_outs.astype(np.float64)
    returns = np.empty((T, N), dtype=np.float64)
    advantage = np.zeros(N, dtype=np.float64)
    for step in reversed(range(T)):
        next_values = last_values.astype(np.float64) if step == T - 1 else values[step + 1]
        next_is_not_terminal = 1.0 - (ended[step] != 0).astype(np.float64)
        delta = rewards[step] + next_is_not_terminal * gamma * next_values - values[step]
        advantage = delta + next_is_not_terminal * gamma * lam * advantage
        returns[step] = advantage + values[step]
    return returns


def gae_recurrence(rew, ended, values, last_values, gamma, lam):
    """navsim_gae_scan's recurrence (include/navsim.h) in float64, float32 store: every episode end terminal"""
    T, N = rew.shape
    gl, gv = np.float64(gamma) * np.float64(lam), np.float64(gamma) * (np.float64(1.0) - np.float64(lam))
    vnext = last_values.astype(np.float32)
    R = vnext.astype(np.float64)
    ret = np.empty((T, N), dtype=np.float32)
    for t in range(T - 1, -1, -1):
        e = ended[t] != 0
        R = (rew[t].astype(np.float64) + np.where(e, 0.0, gv * vnext.astype(np.float64))) + R * np.where(e, 0.0, gl)
        ret[t] = R.astype(np.float32)
        vnext = values[t]
    return ret - values, ret


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_mirror_against_rsl_rl(T, N, lam):
    """|ret - ret_rsl| <= 2^-23 max(|ret_rsl|, 1): one float32 ulp.  The two float64 recurrences agree to ~1e-13 relative to the
    values they carry, so only the mirror's final rounding to float32 (<= 2^-24 relative) can separate them."""
    rew, ended, done, arrive, V, lv = truncated_batch(T, N, seed=int(lam * 100), forced=True)   # (forced rows: also T = 1 holds a time-out)
    trunc = truncated_rows(ended, done, arrive)
    assert trunc.any() and ((arrive != 0) & (ended == 0)).any()
    adv, ret = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv)
    assert adv.dtype == ret.dtype == np.float32 and adv.shape == ret.shape == (T, N)
    want = rsl_rl_returns(rew, ended, trunc, V, lv, GAMMA, lam)
    ratio = np.abs(ret.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
    print(f"T={T} N={N} lam={lam}: {int(trunc.sum())} truncated rows of {int((ended != 0).sum())} ends, worst ratio {ratio.max():.3g}")
    assert ratio.max() <= 2.0 ** -23
    np.testing.assert_array_equal(adv, ret - V)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_mirror_without_a_truncated_row_is_the_gae_recurrence(lam):
    rew, ended, done, arrive, V, lv = truncated_batch(97, 48, seed=5)
    done = np.where(truncated_rows(ended, done, arrive), 1, done).astype(np.uint8)   # every time-out becomes a collision
    assert not truncated_rows(ended, done, arrive).any() and (ended != 0).any()
    adv, ret = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv)
    adv0, ret0 = gae_recurrence(rew, ended, V, lv, GAMMA, lam)
    np.testing.assert_array_equal(ret, ret0)
    np.testing.assert_array_equal(adv, adv0)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_mirror_reductions(lam):
    rew, ended, done, arrive, V, lv = truncated_batch(97, 48, seed=6, forced=True)
    trunc = truncated_rows(ended, done, arrive)
    assert trunc.sum() > 48 and ((ended != 0) & ~trunc).any()
    adv, ret = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv)
    # a truncated row: r + gamma V of the row itself, nothing from behind it
    want = (rew.astype(np.float64) + np.float64(GAMMA) * V.astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(ret[trunc], want[trunc])
    # a terminal end: the reward alone
    term = (ended != 0) & ~trunc
    np.testing.assert_array_equal(ret[term], rew[term])
    # done / arrive without ended change nothing
    free = ended == 0
    assert ((done != 0) & free).any() and ((arrive != 0) & free).any()
    adv1, ret1 = truncated_returns_reference(rew, ended, np.where(free, 0, done), np.where(free, 0, arrive), V, GAMMA, lam, last_value=lv)
    np.testing.assert_array_equal(ret1, ret)
    adv2, ret2 = truncated_returns_reference(rew, ended, np.where(free, 1, done), arrive, V, GAMMA, lam, last_value=lv)
    np.testing.assert_array_equal(ret2, ret)
    adv3, ret3 = truncated_returns_reference(rew, ended, done, np.where(free, 1, arrive), V, GAMMA, lam, last_value=lv)
    np.testing.assert_array_equal(ret3, ret)
    # no last_value = a last_value of zeros
    a, r = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam)
    b, s = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam, last_value=np.zeros(48, np.float32))
    np.testing.assert_array_equal(r, s)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(r, ret)   # (and the bootstrap of the batch end does enter)


# ------------------------------------------------------------------------------------------------ refusals of the C entry point
P = 0x10000   # a non-null, 256-byte aligned address that is never dereferenced: every call below is refused before any HIP call
NAVSIM_E_ARG = -1   # include/navsim.h


def test_gae_scan_trunc_refuses_bad_arguments_without_a_device():
    L = lib()
    f = L.navsim_gae_scan_trunc
    good = dict(rew=P, ended=P, done=P, arrive=P, value=P, last=P, T=8, N=16, gamma=0.99, lam=0.95, adv=P, ret=P, exact=0)
    bad = [dict(rew=None), dict(ended=None), dict(done=None), dict(arrive=None), dict(value=None), dict(adv=None), dict(T=-1), dict(N=-16),
           dict(lam=1.5), dict(lam=-0.01), dict(lam=float("nan")), dict(lam=1.5, exact=1), dict(done=None, N=17)]
    for change in bad:
        a = dict(good, **change)
        rc = f(a["rew"], a["ended"], a["done"], a["arrive"], a["value"], a["last"], a["T"], a["N"], a["gamma"], a["lam"], a["adv"],
               a["ret"], a["exact"], None)
        msg = L.navsim_last_error().decode()
        assert rc == NAVSIM_E_ARG and msg.startswith("navsim_gae_scan_trunc:"), (change, rc, msg)
    # an empty batch is nothing to do, as for navsim_gae_scan (pointers may be null)
    assert f(None, None, None, None, None, None, 0, 16, 0.99, 0.95, None, None, 0, None) == 0
    assert f(None, None, None, None, None, None, 8, 0, 0.99, 0.95, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------------------ configuration and flag
def test_config_default_and_validation():
    assert ppo.PPOConfig().bootstrap_truncated is False
    assert ppo.PPOConfig(bootstrap_truncated=True).bootstrap_truncated is True
    assert ppo.PPOConfig(bootstrap_truncated=True, gae_lambda=0.95, norm_reward=True).gae_lambda == 0.95
    for bad in (1, 0, None, "yes", 1.0, np.bool_(True)):
        with pytest.raises(ValueError, match="bootstrap_truncated"):
            ppo.PPOConfig(bootstrap_truncated=bad)
    cfg = ppo.PPOConfig()
    cfg.bootstrap_truncated = 1   # a config is mutable: the trainer checks again
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        ppo.check_bootstrap_config(cfg)


def test_cli_flag_reaches_the_config():
    assert cli.config_of(cli.get_args(["--bootstrap_truncated"]), 8).bootstrap_truncated is True
    assert cli.config_of(cli.get_args([]), 8).bootstrap_truncated is False
