"""PPOConfig.norm_reward on the GPU: navppo_return_moments against the host mirror at every chunk edge, column tail and episode-end
pattern (same bits on a second call), a rollout split in two against one call, navppo_reward_scale against the merge formula in numpy
(bit-identical outputs given the stored scale; in place; frozen statistics; the prior-dominated clip; an empty and a poisoned batch row),
both entry points inside guarded arenas, two gloo ranks sharing the GPU against one process that plays both, and the trainer end to end."""
import math
import os

import numpy as np
import pytest
import torch

from _guards import canary_of, is_canary, run_both
from _rewards import synthetic_rollout
from navbot_ppo_amd import ppo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F64 = torch.float64
PATTERNS = ("none", "all", "first", "last", "edge", "random")


def _ended(pattern, T, N, seed=0):
    e = np.zeros((T, N), dtype=np.uint8)
    if pattern == "all":
        e[:] = 1
    elif pattern == "first":
        e[0] = 1
    elif pattern == "last":
        e[T - 1] = 1
    elif pattern == "edge":   # both sides of the edge between the first two 32-row chunks: row 31, row 32, or both
        cols = np.arange(N)
        if T > 31:
            e[31, (cols % 2 == 0) | (cols % 5 == 0)] = 1
        if T > 32:
            e[32, (cols % 2 == 1) | (cols % 5 == 0)] = 1
    elif pattern == "random":
        e[:] = np.random.default_rng(seed + 7 * T + N).random((T, N)) < 0.03
    return e


def _fresh_rms():
    return torch.tensor([*ppo.RET_RMS_INIT, 0.0], dtype=F64, device=DEV)


def _assert_moments(got, want, what):
    n, mean, m2 = (float(v) for v in got)
    wn, wmean, wm2 = (float(v) for v in want)
    assert n == wn, what
    assert abs(mean - wmean) <= 1e-12 * math.sqrt(wm2 / wn), (what, mean, wmean)
    assert abs(m2 - wm2) <= 1e-12 * wm2, (what, m2, wm2)


def _assert_stats(got, want, what=""):
    """(mean, var, count) against a reference: the mean within 1e-12 standard deviations, the variance within 1e-12 relative"""
    assert abs(got[0] - want[0]) <= 1e-12 * math.sqrt(want[1]), (what, got, want)
    assert abs(got[1] - want[1]) <= 1e-12 * want[1], (what, got, want)
    assert got[2] == want[2], (what, got, want)


# ------------------------------------------------------------------------------------------------ navppo_return_moments
@pytest.mark.parametrize("N", [1, 5, 16, 37, 64, 100])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 97])
def test_return_moments_match_the_mirror(T, N):
    rew_h, _ = synthetic_rollout(T, N, seed=5)
    rew = torch.from_numpy(rew_h).to(DEV)
    carry_h = np.random.default_rng(T * 1000 + N).normal(0.0, 100.0, N)
    for gamma in (0.99, 1.0, 0.0):
        for k, pattern in enumerate(PATTERNS):
            what = f"T={T} N={N} gamma={gamma} ends={pattern}"
            ended_h = _ended(pattern, T, N)
            ended = torch.from_numpy(ended_h).to(DEV)
            cin = carry_h if k % 2 == 0 else None   # (None: the trainer's case, every column starts at 0)
            want = ppo.reward_norm_reference(rew_h, ended_h, gamma, carry=cin)
            runs = []
            for _ in range(2):
                carry = None if cin is None else torch.from_numpy(cin).to(DEV)
                runs.append((ppo.return_moments(rew, ended, gamma, carry=carry), carry))
            (m, carry), (m2, carry2) = runs
            assert torch.equal(m, m2) and (carry is None or torch.equal(carry, carry2)), what   # the same call, the same bits
            _assert_moments(m.tolist(), want.moments, what)
            if carry is not None:
                got = carry.cpu().numpy()
                assert (np.abs(got - want.carry) <= 1e-12 * np.abs(want.carry)).all(), (what, np.abs(got - want.carry).max())
                assert (got[ended_h[T - 1] != 0] == 0.0).all(), what


@pytest.mark.parametrize("N", [37, 64])
def test_a_rollout_split_in_two_gives_the_statistics_of_one_call(N):
    T, cut, gamma = 97, 49, 0.99
    rew_h, ended_h = synthetic_rollout(T, N, seed=9, p_end=0.03)
    rew, ended = torch.from_numpy(rew_h).to(DEV), torch.from_numpy(ended_h).to(DEV)
    rows = torch.zeros((2, 3), dtype=F64, device=DEV)
    carry = torch.zeros(N, dtype=F64, device=DEV)
    ppo.return_moments(rew[:cut], ended[:cut], gamma, carry=carry, out=rows[0])
    ppo.return_moments(rew[cut:], ended[cut:], gamma, carry=carry, out=rows[1])
    two, one = _fresh_rms(), _fresh_rms()
    ppo.reward_scale(two, rows, rew)
    whole = ppo.return_moments(rew, ended, gamma)
    ppo.reward_scale(one, whole, rew)
    assert float(rows[0, 0]) == cut * N and float(rows[1, 0]) == (T - cut) * N
    _assert_stats(two.tolist(), one.tolist())
    _assert_stats(two.tolist(), ppo.reward_norm_reference(rew_h, ended_h, gamma).rms)
    want = ppo.reward_norm_reference(rew_h, ended_h, gamma).carry
    assert (np.abs(carry.cpu().numpy() - want) <= 1e-12 * np.abs(want)).all()


# ------------------------------------------------------------------------------------------------ navppo_reward_scale
def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def _batch_rows():
    """two batch rows as the kernel produces them (a 33 x 5 and a 97 x 64 rollout)"""
    rows = torch.zeros((2, 3), dtype=F64, device=DEV)
    for k, (T, N) in enumerate(((33, 5), (97, 64))):
        r, e = synthetic_rollout(T, N, seed=11 + k)
        ppo.return_moments(torch.from_numpy(r).to(DEV), torch.from_numpy(e).to(DEV), 0.99, out=rows[k])
    return rows


def _mirror_scaled(rew_h, scale, clip):
    return np.clip((rew_h.astype(np.float64) * np.float64(scale)).astype(np.float32), np.float32(-clip), np.float32(clip))


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_reward_scale_merges_and_scales(n, inplace):
    clip, eps = 0.125, 1e-8   # (a bound that many of the scaled rewards reach, and not all)
    rows = _batch_rows()
    rew_h = synthetic_rollout(1, n, seed=21)[0].reshape(n)
    rew = torch.from_numpy(rew_h).to(DEV)
    rms = _fresh_rms()
    out = ppo.reward_scale(rms, rows, rew, clip=clip, eps=eps, out=rew if inplace else None)
    assert (out is rew) == inplace
    mean, var, count, scale = rms.tolist()
    _assert_stats((mean, var, count), ppo.merge_return_moments(ppo.RET_RMS_INIT, rows.cpu().numpy()))
    assert _ulps(scale, 1.0 / np.sqrt(np.float64(var) + eps)) <= 4
    assert np.array_equal(out.cpu().numpy().view(np.int32), _mirror_scaled(rew_h, scale, clip).view(np.int32))
    assert n < 63 or (float(out.abs().max()) == clip and float(out.abs().min()) < clip)
    # K = 0: frozen statistics, bit for bit; the same scale again
    kept = rms.clone()
    again = ppo.reward_scale(rms, None, torch.from_numpy(rew_h).to(DEV), clip=clip, eps=eps)
    assert torch.equal(rms.view(torch.int64), kept.view(torch.int64)) and torch.equal(again, out)


def test_a_prior_dominated_single_return_clips():
    rew = torch.tensor([[7.0]], device=DEV)
    m = ppo.return_moments(rew, torch.zeros((1, 1), dtype=torch.uint8, device=DEV), 0.99)
    assert m.tolist() == [1.0, 7.0, 0.0]
    rms = _fresh_rms()
    out = ppo.reward_scale(rms, m, rew)
    want = ppo.reward_norm_reference(np.array([[7.0]], dtype=np.float32), np.zeros((1, 1)), 0.99)
    _assert_stats(rms.tolist(), want.rms)
    assert 13.0 < float(rms[3]) < 15.0 and _ulps(float(rms[3]), want.rms[3]) <= 4   # one return against a prior of count 1e-4
    assert out.tolist() == [[10.0]] and want.out.tolist() == [[10.0]]


def test_an_empty_row_and_a_poisoned_batch_leave_the_statistics_alone():
    T, N = 33, 16
    rew_h, ended_h = synthetic_rollout(T, N, seed=31)
    rew, ended = torch.from_numpy(rew_h).to(DEV), torch.from_numpy(ended_h).to(DEV)
    rms = _fresh_rms()
    ppo.reward_scale(rms, ppo.return_moments(rew, ended, 0.99), rew)   # one good batch first
    kept = rms.clone()
    bad_h = rew_h.copy()
    bad_h[17, 3] = np.nan
    bad = torch.from_numpy(bad_h).to(DEV)
    rows = torch.zeros((2, 3), dtype=F64, device=DEV)
    rows[0] = torch.tensor([0.0, 5.0, 5.0], dtype=F64)   # bn = 0
    ppo.return_moments(bad, ended, 0.99, out=rows[1])
    assert float(rows[1, 0]) == T * N and math.isnan(float(rows[1, 1]))
    out = ppo.reward_scale(rms, rows, bad)
    assert torch.equal(rms.view(torch.int64), kept.view(torch.int64))
    got, want = out.cpu().numpy(), _mirror_scaled(bad_h, float(kept[3]), 10.0)
    assert np.isnan(got[17, 3]) and np.isnan(got).sum() == 1   # the trainer's non-finite guard still sees it
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------ guarded arenas
@pytest.mark.parametrize("N", [37, 64])
def test_return_moments_inside_guards(N):
    T, gamma = 97, 0.99
    rew_h, ended_h = synthetic_rollout(T, N, seed=41, p_end=0.03)
    cin = np.random.default_rng(N).normal(0.0, 100.0, N)
    want = ppo.reward_norm_reference(rew_h, ended_h, gamma, carry=cin)

    def call(g):
        rew, ended = g.inp(torch.from_numpy(rew_h), 4), g.inp(torch.from_numpy(ended_h), 1)
        carry = g.io(torch.from_numpy(cin), 8)
        m = g.out((3,), F64, 8)
        ppo.return_moments(rew, ended, gamma, carry=carry, out=m)
        return m, carry

    m, carry = run_both(DEV, call, f"navppo_return_moments N={N}")   # guards intact, no canary in moments, both placements equal
    _assert_moments(m.tolist(), want.moments, N)
    assert (np.abs(carry.cpu().numpy() - want.carry) <= 1e-12 * np.abs(want.carry)).all()


@pytest.mark.parametrize("inplace", [False, True])
def test_reward_scale_inside_guards(inplace):
    n = 4099
    rows_h = _batch_rows().cpu()
    rew_h = torch.from_numpy(synthetic_rollout(1, n, seed=43)[0].reshape(n))
    rms_h = torch.tensor([*ppo.RET_RMS_INIT, 0.0], dtype=F64)
    rms_h.view(torch.int64)[3] = canary_of(F64).view(torch.int64)[0]   # the scale slot holds the canary: the call must replace it

    def call(g):
        rms, rows = g.io(rms_h, 8), g.inp(rows_h, 8)
        rew = g.io(rew_h, 4) if inplace else g.inp(rew_h, 4)
        out = rew if inplace else g.out((n,), torch.float32, 4)
        ppo.reward_scale(rms, rows, rew, out=out)
        return rms, out

    rms, out = run_both(DEV, call, f"navppo_reward_scale inplace={inplace}")
    assert not bool(is_canary(rms).any()) and not bool(is_canary(out).any())
    assert np.array_equal(out.cpu().numpy().view(np.int32), _mirror_scaled(rew_h.numpy(), float(rms[3]), 10.0).view(np.int32))


# ------------------------------------------------------------------------------------------------ two ranks
def _bare_trainer(rew, ended, ctx, world):
    """what PPOTrainer._normalise_rewards touches, without an env: the trainer's own multi-rank code runs"""
    t = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    t.cfg, t.ctx = ppo.PPOConfig(norm_reward=True), ctx
    t.rew_buf, t.ended_buf = rew, ended
    t.rew_scaled_buf = torch.zeros_like(rew)
    t._ret_rows = torch.zeros((world, 3), dtype=F64, device=DEV)
    t._init_ret_rms(DEV)
    return t


def _halves(rank):
    rew_h, ended_h = synthetic_rollout(97, 96, seed=51, p_end=0.03)
    sl = slice(rank * 48, (rank + 1) * 48)
    return torch.from_numpy(np.ascontiguousarray(rew_h[:, sl])).to(DEV), torch.from_numpy(np.ascontiguousarray(ended_h[:, sl])).to(DEV)


def _rn_rank_worker(rank, world, port, path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduce here
    ctx = ppo.DistCtx(device="cuda:0")
    t = _bare_trainer(*_halves(rank), ctx, world)
    for _ in range(2):   # two rollouts' worth: the second merge starts from shared statistics
        out = t._normalise_rewards()
    torch.cuda.synchronize()
    torch.save({"rms": t.ret_rms.cpu(), "rows": t._ret_rows.cpu(), "out": out.cpu()}, f"{path}.{rank}")
    ctx.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_hold_the_statistics_of_one_process_that_plays_both(tmp_path):
    from _ranks import spawn_ranks
    path = str(tmp_path / "rn")
    spawn_ranks(_rn_rank_worker, 2, lambda port: (2, port, path))
    r0, r1 = torch.load(path + ".0"), torch.load(path + ".1")
    assert torch.equal(r0["rms"].view(torch.int64), r1["rms"].view(torch.int64)) and torch.equal(r0["rows"], r1["rows"])
    halves = [_halves(r) for r in range(2)]
    rows = torch.zeros((2, 3), dtype=F64, device=DEV)
    for r, (rew, ended) in enumerate(halves):
        ppo.return_moments(rew, ended, 0.99, out=rows[r])
    rms = _fresh_rms()
    for _ in range(2):
        outs = [ppo.reward_scale(rms, rows if r == 0 else None, halves[r][0]) for r in range(2)]   # (one merge per rollout)
    assert torch.equal(rows.cpu(), r0["rows"]) and torch.equal(rms.cpu().view(torch.int64), r0["rms"].view(torch.int64))
    assert torch.equal(outs[0].cpu(), r0["out"]) and torch.equal(outs[1].cpu(), r1["out"])
    count = 1e-4
    for _ in range(4):   # two rollouts of two rows of 97 x 48 returns, added in the order of the merges
        count += 97 * 48
    assert float(rms[2]) == count


# ------------------------------------------------------------------------------------------------ the trainer
NEW_KEYS = ("reward_scale", "ret_rms_mean", "ret_rms_std", "explained_variance")


def _trainer(policy, **cfg):
    from navbot_ppo_amd.env import VecEnv
    env = VecEnv(64, map="stage_1", max_episode_steps=12, seed=1)
    return ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=32, max_episode_steps=12, n_updates_per_iteration=2, policy=policy, seed=2, **cfg))


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_scales_what_the_scan_reads_and_nothing_else(policy):
    from navbot_ppo_amd.env import rtg_scan
    on, off = _trainer(policy, norm_reward=True), _trainer(policy)
    lg_on, lg_off = on.iteration(), off.iteration()
    for name in ("obs_buf", "act_buf", "rew_buf", "ended_buf"):   # the option does not touch the rollout
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    assert not any(k in lg_off for k in NEW_KEYS) and not hasattr(off, "ret_rms") and not hasattr(off, "rew_scaled_buf")
    assert not any(k.startswith("ppo/re") or k == "ppo/explained_variance" for k in off.tb_scalars())
    rolls = [(on.rew_buf.cpu().numpy().copy(), on.ended_buf.cpu().numpy().copy())]
    scale = float(on.ret_rms[3])
    scaled = torch.from_numpy(_mirror_scaled(rolls[0][0], scale, 10.0)).to(DEV)
    assert torch.equal(on.rew_scaled_buf, scaled)
    assert torch.equal(on.rtg_buf, rtg_scan(scaled, on.ended_buf, on.cfg.gamma))   # the unchanged scan, on the scaled buffer
    assert not torch.equal(on.rtg_buf, off.rtg_buf) and lg_on["critic_loss"] < lg_off["critic_loss"]
    lg = on.iteration()
    rolls.append((on.rew_buf.cpu().numpy(), on.ended_buf.cpu().numpy()))
    want = ppo.RET_RMS_INIT
    for rew_h, ended_h in rolls:
        want = ppo.reward_norm_reference(rew_h, ended_h, on.cfg.gamma, rms=want[:3]).rms
    _assert_stats(on.ret_rms.tolist(), want)
    assert lg["iteration"] == 2 and all(math.isfinite(lg[k]) for k in NEW_KEYS + ("actor_loss", "critic_loss", "approx_kl"))
    assert lg["reward_scale"] == float(on.ret_rms[3]) and lg["ret_rms_mean"] == float(on.ret_rms[0])
    assert lg["ret_rms_std"] == math.sqrt(float(on.ret_rms[1])) and lg["explained_variance"] <= 1.0
    assert all("ppo/" + k in on.tb_scalars() for k in NEW_KEYS)
    # the episode figures are raw: the mean of the kernels' own episode returns over the episodes that ended
    ended = on.ended_buf.bool()
    assert int(ended.sum()) == lg["episodes"] > 0
    assert lg["avg_ep_rews"] == pytest.approx(float(on.epret_buf[ended].double().mean()), rel=1e-9)
    on.env.close()
    off.env.close()


def test_trainer_with_gae_runs_on_the_scaled_rewards():
    tr = _trainer("mlp64x2", norm_reward=True, gae_lambda=0.95)
    lg = tr.iteration()
    assert all(math.isfinite(lg[k]) for k in NEW_KEYS + ("actor_loss", "critic_loss"))
    scaled = torch.from_numpy(_mirror_scaled(tr.rew_buf.cpu().numpy(), float(tr.ret_rms[3]), 10.0)).to(DEV)
    assert torch.equal(tr.rew_scaled_buf, scaled)
    assert bool(torch.isfinite(tr.rtg_buf).all()) and bool(torch.isfinite(tr._gae[0]).all())
    tr.env.close()
