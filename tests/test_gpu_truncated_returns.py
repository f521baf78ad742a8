"""navsim_gae_scan_trunc and PPOConfig.bootstrap_truncated on the device, against the host mirror env.truncated_returns_reference.

Contract (include/navsim.h): the serial kernel (N % 16 != 0, or exact) is the mirror bit for bit; the T-split kernel is within one
float32 ulp of it and bit-identical on every row with `ended` set; without a time-out both are navsim_gae_scan's outputs bit for bit.
The batches (tests/_truncation.py) carry a time-out on the first and last row, on both sides of every 32-row chunk edge and of the
512-row super-chunk edge, twice inside one chunk and on the row before a collision, beside done / arrive rows without an episode end."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _guards import run_both
from _truncation import truncated_batch, truncated_rows
from navbot_ppo_amd import ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import gae_scan, gae_scan_trunc, rtg_scan, truncated_returns_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GAMMA = 0.99
LAMBDAS = [0.0, 0.95, 1.0]
SPLIT_SHAPES = [(1, 16), (31, 16), (32, 16), (33, 48), (512, 16), (513, 16), (545, 1024)]   # 1024 columns: 64 workgroups, the XCD remap
SERIAL_SHAPES = [(T, N) for N in (1, 17, 100) for T in (1, 33, 513)]


@functools.lru_cache(maxsize=None)
def _batch(T, N):
    b = truncated_batch(T, N, seed=11, forced=True)
    trunc = truncated_rows(*b[1:4])
    term = (b[1] != 0) & ~trunc
    if T == 1:
        assert trunc.any() or term.any()
    else:
        assert trunc.any() and term.any()
    if N >= 7:   # all seven families of forced rows exist
        assert trunc[0].any() and trunc[T - 1].any()
        assert ((b[3] != 0) & (b[1] == 0)).any() and ((b[2] != 0) & (b[1] == 0)).any() or T == 1
    return b


@functools.lru_cache(maxsize=None)
def _mirror(T, N, lam, with_last):
    """(adv, ret) of the mirror as device tensors, computed once per case and shared (never written)"""
    rew, ended, done, arrive, V, lv = _batch(T, N)
    adv, ret = truncated_returns_reference(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv if with_last else None)
    return torch.from_numpy(adv).to(DEV), torch.from_numpy(ret).to(DEV)


def _dev(T, N):
    return [torch.from_numpy(a).to(DEV) for a in _batch(T, N)]


def assert_within_one_ulp(got, want, what):
    lo = torch.nextafter(want, torch.full_like(want, -float("inf")))
    hi = torch.nextafter(want, torch.full_like(want, float("inf")))
    bad = ~((got >= lo) & (got <= hi))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) more than one float32 ulp from the mirror"


@pytest.mark.parametrize("with_last", [True, False])
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("T,N", SERIAL_SHAPES + [(33, 16)])
def test_serial_kernel_is_the_mirror(T, N, lam, with_last):
    rew, ended, done, arrive, V, lv = _dev(T, N)
    adv, ret = gae_scan_trunc(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv if with_last else None, exact=N % 16 == 0)
    want_adv, want_ret = _mirror(T, N, lam, with_last)
    assert torch.equal(ret, want_ret) and torch.equal(adv, want_adv)
    adv2, none = gae_scan_trunc(rew, ended, done, arrive, V, GAMMA, lam, last_value=lv if with_last else None, exact=N % 16 == 0,
                                want_returns=False)
    assert none is None and torch.equal(adv2, adv)


@pytest.mark.parametrize("with_last", [True, False])
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("T,N", SPLIT_SHAPES)
def test_split_kernel_within_one_ulp(T, N, lam, with_last):
    rew, ended, done, arrive, V, lv = _dev(T, N)
    last = lv if with_last else None
    adv, ret = gae_scan_trunc(rew, ended, done, arrive, V, GAMMA, lam, last_value=last)
    want_adv, want_ret = _mirror(T, N, lam, with_last)
    n_off = int((ret != want_ret).sum())
    print(f"T={T} N={N} lam={lam} last_value={with_last}: {n_off} of {T * N} stores differ from the mirror")
    assert_within_one_ulp(ret, want_ret, f"T={T} N={N} lam={lam}")
    e = ended != 0
    assert torch.equal(ret[e], want_ret[e])          # the factor is 0 there: the carry-in does not enter
    assert torch.equal(adv, ret - V)                 # the kernel's own float32 return minus V
    adv2, none = gae_scan_trunc(rew, ended, done, arrive, V, GAMMA, lam, last_value=last, want_returns=False)
    assert none is None and torch.equal(adv2, adv)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("T,N", SPLIT_SHAPES + SERIAL_SHAPES)
def test_without_a_time_out_it_is_gae_scan(T, N, lam):
    rew, ended, done, arrive, V, lv = _dev(T, N)
    trunc = (ended != 0) & (done == 0) & (arrive == 0)
    done = torch.where(trunc, torch.ones_like(done), done)   # every time-out rewritten as a collision
    for exact in (False, True):
        for last in (lv, None):
            adv, ret = gae_scan_trunc(rew, ended, done, arrive, V, GAMMA, lam, last_value=last, exact=exact)
            adv0, ret0 = gae_scan(rew, ended, V, GAMMA, lam, last_value=last, exact=exact)
            assert torch.equal(ret, ret0) and torch.equal(adv, adv0), (exact, last is None)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("T,N", [(33, 48), (33, 17)])
def test_guarded_buffers(T, N):
    """every argument inside a guarded allocation, at a 256-byte boundary and at its minimum alignment (4 bytes for float buffers, 1 for
    flags): the ragged first chunk's rows t < 0 are loaded from row 0, not from in front of the buffers"""
    L = lib()
    b = _dev(T, N)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lam, with_last in ((0.95, True), (1.0, False)):
        def call(g):
            rew, ended, done, arrive, V, lv = (g.inp(t, 1 if t.dtype == torch.uint8 else 4) for t in b)
            adv, ret = g.out((T, N), torch.float32, 4), g.out((T, N), torch.float32, 4)
            assert L.navsim_gae_scan_trunc(P(rew), P(ended), P(done), P(arrive), P(V), P(lv) if with_last else None, T, N, GAMMA, lam, P(adv),
                                           P(ret), 0, st) == 0
            return adv, ret

        adv, ret = run_both(DEV, call, f"gae_scan_trunc T={T} N={N} lam={lam}")
        want_adv, want_ret = _mirror(T, N, lam, with_last)
        if N % 16:
            assert torch.equal(ret, want_ret) and torch.equal(adv, want_adv)
        else:
            assert_within_one_ulp(ret, want_ret, f"guarded T={T} N={N}")
            assert torch.equal(adv, ret - b[4])


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(policy, **cfg):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(64, map="stage_1", max_episode_steps=20, seed=1)
    return ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=48, max_episode_steps=20, n_updates_per_iteration=1, policy=policy, seed=2, **cfg))


def assert_net_rows_are_the_rule(tr):
    """PPOConfig.scan_history: the rows the nets read -- all T + 1 of them, the last one bootstraps the batch end -- are
    stack_rows_reference of the trainer's own obs_buf / ended_buf, bit for bit; without it they are obs_buf itself"""
    if not tr.scan_history:
        assert tr.net_obs is tr.obs_buf and tr.net_dim == tr.env.D
        return
    from navbot_ppo_amd.env import HIST_DIM, stack_rows_reference
    want = torch.from_numpy(stack_rows_reference(tr.obs_buf.cpu().numpy(), tr.ended_buf.cpu().numpy()))
    assert tr.net_obs is tr.hist_buf and tr.net_dim == HIST_DIM and tr.hist_buf.shape == want.shape
    assert tr.hist_buf.dtype == want.dtype and torch.equal(tr.hist_buf.cpu().view(torch.uint8), want.view(torch.uint8))


# (scan_history rides on the policy: it exists for mlp64x2 only)
@pytest.mark.parametrize("norm_reward", [False, True])
@pytest.mark.parametrize("gae_lambda", [None, 0.95])
@pytest.mark.parametrize("policy,scan_history", [("mlp64x2", False), ("resmlp512", False), ("mlp64x2", True)],
                         ids=["mlp64x2", "resmlp512", "mlp64x2+history"])
def test_trainer_targets_are_the_mirror_of_its_own_buffers(policy, scan_history, gae_lambda, norm_reward):
    """A fresh policy drives at most 0.25 m/s x 0.2 s x 20 steps = 1 m per episode, so nearly every episode of the 20-step limit is cut
    by it (the CPU oracle counts 127-128 truncated rows in 64 x 48 for random actions): two time-outs per env, and the batch end cuts
    the third episode of every env.  With scan_history V is taken on the T + 1 history rows."""
    T, N = 48, 64
    tr = _trainer(policy, bootstrap_truncated=True, gae_lambda=gae_lambda, norm_reward=norm_reward, scan_history=scan_history)
    tr.rollout()
    ended, done, arrive = (t.cpu().numpy() for t in (tr.ended_buf, tr.done_buf, tr.arrive_buf))
    n_trunc = int(truncated_rows(ended, done, arrive).sum())
    assert n_trunc >= N, n_trunc                      # what keeps the test honest: the rule is exercised ...
    assert int((ended[T - 1] == 0).sum()) >= 1        # ... and so is the bootstrap of the batch end
    rew = tr.rew_scaled_buf if norm_reward else tr.rew_buf
    assert_net_rows_are_the_rule(tr)
    Vall = tr.updater.value(tr.net_obs.reshape(-1, tr.net_dim)).reshape(T + 1, N)
    want_adv, want_ret = truncated_returns_reference(rew.cpu().numpy(), ended, done, arrive, Vall[:T].cpu().numpy(), tr.cfg.gamma,
                                                     1.0 if gae_lambda is None else gae_lambda, last_value=Vall[T].cpu().numpy())
    want_ret = torch.from_numpy(want_ret).to(DEV)
    assert_within_one_ulp(tr.rtg_buf, want_ret, "rtg_buf")
    assert tr._gae is not None and torch.equal(tr._gae[1], Vall[:T].reshape(-1))
    assert torch.equal(tr._gae[0], tr.rtg_buf.reshape(-1) - tr._gae[1])   # adv = the scan's own return minus V
    e = torch.from_numpy(ended != 0).to(DEV)
    assert torch.equal(tr.rtg_buf[e], want_ret[e])
    assert torch.equal(torch.from_numpy(want_adv).to(DEV)[e], tr._gae[0].reshape(T, N)[e])
    lg = tr.iteration()
    assert lg["bootstrapped_frac"] > 0 and lg["bootstrapped_frac"] == lg["timeouts"] / (T * N)
    assert tr.tb_scalars()["ppo/bootstrapped_frac"] == lg["bootstrapped_frac"]
    assert np.isfinite(lg["actor_loss"]) and np.isfinite(lg["critic_loss"])


@pytest.mark.parametrize("norm_reward", [False, True])
@pytest.mark.parametrize("gae_lambda,scan_history", [(None, False), (0.95, False), (None, True), (0.95, True)],
                         ids=["None", "0.95", "None+history", "0.95+history"])
def test_trainer_with_the_option_off_is_todays(gae_lambda, scan_history, norm_reward):
    T, N = 48, 64
    tr = _trainer("mlp64x2", gae_lambda=gae_lambda, norm_reward=norm_reward, scan_history=scan_history)
    assert tr.cfg.bootstrap_truncated is False
    tr.rollout()
    rew = tr.rew_scaled_buf if norm_reward else tr.rew_buf
    assert_net_rows_are_the_rule(tr)
    if gae_lambda is None:
        assert tr._gae is None and torch.equal(tr.rtg_buf, rtg_scan(rew, tr.ended_buf, tr.cfg.gamma))
    else:
        Vall = tr.updater.value(tr.net_obs.reshape(-1, tr.net_dim)).reshape(T + 1, N)
        adv, ret = gae_scan(rew, tr.ended_buf, Vall[:T].contiguous(), tr.cfg.gamma, gae_lambda, last_value=Vall[T])
        assert torch.equal(tr.rtg_buf, ret) and torch.equal(tr._gae[0], adv.reshape(-1))
    lg = tr.iteration()
    assert "bootstrapped_frac" not in lg and "ppo/bootstrapped_frac" not in tr.tb_scalars()


def test_trainer_refuses_a_non_bool_option():
    from navbot_ppo_amd.env import VecEnv
    cfg = ppo.PPOConfig(rollout_len=8, max_episode_steps=8, policy="mlp64x2")
    cfg.bootstrap_truncated = 1
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        ppo.PPOTrainer(VecEnv(16, map="stage_1", max_episode_steps=8, seed=1), cfg)
