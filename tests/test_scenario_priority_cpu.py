"""Scenario-prioritised training, the host side (no GPU): the mirror of navppo_group_sums against a brute-force loop, the rule of
ScenarioSampler, the refusals of the options and the checkpoint's sidecar."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

from navbot_ppo_amd import ppo
from navbot_ppo_amd.scenarios import ScenarioSampler, group_sums_reference


# ---------------------------------------------------------------- 1. group_sums_reference
def _buffers(T, N, K, seed, lo=0, hi=None):
    """random [T, N] rollout buffers with all four episode outcomes (and flags set on rows that did not end: they must not count)"""
    rng = np.random.default_rng(seed)
    ended = (rng.random((T, N)) < 0.3).astype(np.uint8)
    arrive = (rng.random((T, N)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (T, N)).astype(np.uint8)
    done = (rng.random((T, N)) < 0.5).astype(np.uint8)
    ep_length = rng.integers(0, 500, (T, N)).astype(np.int32)
    ep_return = (rng.standard_normal((T, N)) * 100).astype(np.float32)
    adv = rng.standard_normal((T, N)).astype(np.float32)
    group = rng.integers(lo, K if hi is None else hi, N).astype(np.int32)
    return ended, arrive, done, ep_length, ep_return, adv, group


def _brute(ended, arrive, done, ep_length, ep_return, group, K, adv=None):
    T, N = ended.shape
    out = [[0.0] * 8 for _ in range(K)]
    for n in range(N):
        k = int(group[n])
        if not 0 <= k < K:
            continue
        out[k][7] += T
        for t in range(T):
            out[k][4] += int(ep_length[t, n])
            if adv is not None:
                out[k][6] += abs(float(adv[t, n]))
            if ended[t, n]:
                out[k][0] += 1
                out[k][5] += float(ep_return[t, n])
                if arrive[t, n]:
                    out[k][1] += 1
                elif done[t, n]:
                    out[k][2] += 1
                else:
                    out[k][3] += 1
    return np.asarray(out)


@pytest.mark.parametrize("with_adv", [False, True])
def test_group_sums_reference_against_a_brute_force_loop(with_adv):
    T, N, K = 13, 29, 5
    e, a, d, ln, rt, adv, g = _buffers(T, N, K, 3, lo=-1, hi=K + 1)   # ids -1 and K among them: counted nowhere
    g[g == 3] = 1                                                      # ... and group 3 has no env: a zero row
    got = group_sums_reference(e, a, d, ln, rt, g, K, adv=adv if with_adv else None)
    want = _brute(e, a, d, ln, rt, g, K, adv if with_adv else None)
    assert got.shape == (K, 8) and got.dtype == np.float64
    assert np.array_equal(got[:, [0, 1, 2, 3, 4, 7]], want[:, [0, 1, 2, 3, 4, 7]])
    np.testing.assert_allclose(got[:, 5:7], want[:, 5:7], rtol=1e-13, atol=1e-9)
    assert not got[3].any() and (got[:, 7].sum() == T * np.isin(g, range(K)).sum())
    # all four outcomes occur, and the outcomes partition the episodes
    assert (got[:, :4].sum(axis=0) > 0).all() and np.array_equal(got[:, 0], got[:, 1:4].sum(axis=1))
    assert with_adv == bool(got[:, 6].any())


# ---------------------------------------------------------------- 2. ScenarioSampler
def _sums(K, episodes, successes, adv_sum=None, rows=None):
    G = np.zeros((K, 8))
    G[:, 0], G[:, 1] = episodes, successes
    G[:, 6] = 0 if adv_sum is None else adv_sum
    G[:, 7] = G[:, 0] if rows is None else rows
    return G


def _scored(K=7, seed=0, **kw):
    s = ScenarioSampler(K, seed=seed, **kw)
    s.observe(_sums(K, 10, [9, 1, 5, 5, 0, 10, 3]))   # failure: .1 .9 .5 .5 1. 0. .7
    return s


def test_counts_sum_to_the_envs_and_every_scenario_plays():
    for n in (7, 8, 48, 100, 4096):
        c = _scored().counts(n)
        assert c.sum() == n and c.min() >= 1, (n, c)
    with pytest.raises(ValueError, match="at least one env"):
        _scored().counts(6)


def test_ranks_ties_to_the_lower_id_and_counts_fall_with_the_rank():
    s = _scored()
    assert s.ranks().tolist() == [6, 2, 4, 5, 1, 7, 3]          # scores 1. .9 .7 .5 .5 .1 0.: the tie at .5 goes to id 2
    for n in (48, 4096):
        c = s.counts(n)
        by_rank = c[np.argsort(s.ranks())]
        assert (np.diff(by_rank) <= 0).all(), by_rank
        assert by_rank[0] > by_rank[-1]
    w = s.weights()
    assert abs(w.sum() - 1) < 1e-12 and w.min() >= 0.25 / 7 - 1e-15
    p = (1.0 / s.ranks()) ** (1 / 0.3)
    np.testing.assert_allclose(w, 0.75 * p / p.sum() + 0.25 / 7, rtol=1e-14)


def test_uniform_mix_one_gives_counts_that_differ_by_at_most_one():
    s = _scored(uniform_mix=1.0)
    for n in (7, 48, 100, 4099):
        c = s.counts(n)
        assert c.sum() == n and c.max() - c.min() <= 1, c
        assert (np.diff(c) <= 0).all()       # the spare envs go to the lower ids


def test_without_the_uniform_floor_a_tie_goes_to_the_lower_id():
    """uniform_mix = 0: the weights are the rank weights alone -- nothing lifts the tail.  Scenarios 2 and 3 tie at .5: the lower id
    ranks first and, wherever the weights give the two a different count, gets the larger one; every scenario still plays."""
    s = _scored(uniform_mix=0.0)
    assert s.score[2] == s.score[3] and s.ranks()[2] + 1 == s.ranks()[3]
    p = (1.0 / s.ranks()) ** (1 / 0.3)
    np.testing.assert_allclose(s.weights(), p / p.sum(), rtol=1e-14)
    assert abs(s.weights().sum() - 1) < 1e-12 and s.weights().min() < 0.25 / 7
    for n in (7, 8, 48, 4096):
        c = s.counts(n)
        assert c.sum() == n and c.min() >= 1, (n, c)
        assert (np.diff(c[np.argsort(s.ranks())]) <= 0).all(), (n, c)
        assert c[2] >= c[3], (n, c)
    assert s.counts(4096)[2] > s.counts(4096)[3]
    assert np.array_equal(np.bincount(s.assign(48), minlength=7), _scored(uniform_mix=0.0).counts(48))
    # every score the same: the ranks are the ids, the counts fall with the id
    t = ScenarioSampler(5, uniform_mix=0.0)
    t.observe(_sums(5, 10, 5))
    assert t.ranks().tolist() == [1, 2, 3, 4, 5]
    for n in (5, 6, 33, 1000):
        c = t.counts(n)
        assert c.sum() == n and c.min() >= 1 and (np.diff(c) <= 0).all(), (n, c)
    # ... and with the floor alone nobody is preferred beyond the spare envs
    u = ScenarioSampler(5, uniform_mix=1.0)
    u.observe(_sums(5, 10, 5))
    assert u.counts(33).tolist() == [7, 7, 7, 6, 6]


def test_more_scenarios_than_envs_are_refused_not_left_without_an_env():
    """K > N: some scenario would get no env, and its statistics would never be measured again: assign refuses -- for the whole run
    and for a shard alike -- and counts nothing; K == N is one env each"""
    s = _scored()
    for kw in (dict(), dict(env_id_base=0, n_envs=3), dict(env_id_base=3, n_envs=3)):
        with pytest.raises(ValueError, match="6 envs cannot play 7 scenarios"):
            s.assign(6, **kw)
    assert s.counter == 0
    ids = s.assign(7)
    assert sorted(ids.tolist()) == list(range(7)) and s.counter == 1
    assert _scored(uniform_mix=0.0).counts(7).tolist() == [1] * 7


def test_first_sight_then_the_exponential_average_and_unobserved_scores_stay():
    s = ScenarioSampler(3, alpha=0.25)
    assert np.isnan(s.score).all()
    s.observe(_sums(3, [10, 0, 4], [5, 0, 4]))
    assert s.score[0] == 0.5 and np.isnan(s.score[1]) and s.score[2] == 0.0
    s.observe(_sums(3, [10, 8, 0], [10, 2, 0]))
    assert s.score[0] == 0.75 * 0.5 + 0.25 * 0.0       # the average
    assert s.score[1] == 0.75                          # first sight: the raw score
    assert s.score[2] == 0.0                           # not observed: kept
    a = ScenarioSampler(2, mode="abs_adv", alpha=1.0)
    a.observe(_sums(2, 0, 0, adv_sum=[6.0, 1.0], rows=[4, 0]))
    assert a.score[0] == 1.5 and np.isnan(a.score[1])  # rows, not episodes, decide what abs_adv observed


def test_unset_scores_rank_first():
    s = ScenarioSampler(4)
    s.observe(_sums(4, [5, 0, 5, 0], [0, 0, 5, 0]))     # scores 1., unset, 0., unset
    assert s.ranks().tolist() == [3, 1, 4, 2]
    c = s.counts(40)
    assert c[1] >= c[3] >= c[0] >= c[2]


def test_the_assignment_is_deterministic_and_realises_the_counts():
    a, b = _scored(), _scored()
    ia, ib = a.assign(100), b.assign(100)
    assert ia.dtype == np.int32 and np.array_equal(ia, ib)
    assert np.array_equal(np.bincount(ia, minlength=7), _scored().counts(100))
    assert a.counter == 1
    assert not np.array_equal(ia, _scored(seed=1).assign(100))     # the seed is part of the hash
    assert not np.array_equal(ia, np.sort(ia))                     # spread over the ids, not laid out in blocks


def test_shards_concatenate_to_the_single_run():
    whole = _scored().assign(96)
    parts = []
    for r in range(4):
        s = _scored()
        parts.append(s.assign(96, env_id_base=24 * r, n_envs=24))
        assert parts[-1].shape == (24,)
    assert np.array_equal(np.concatenate(parts), whole)
    with pytest.raises(ValueError, match="outside"):
        _scored().assign(96, env_id_base=90, n_envs=24)


def test_another_counter_another_permutation():
    s = _scored()
    first, second = s.assign(64), s.assign(64)
    assert s.counter == 2
    assert np.array_equal(np.bincount(first), np.bincount(second))   # the same counts (nothing was observed in between)
    assert not np.array_equal(first, second)
    assert sorted(s.permutation(64).tolist()) == list(range(64))


def test_sampler_state_round_trip():
    s = _scored()
    s.assign(20)
    t = ScenarioSampler(7)
    t.load_state_dict(s.state_dict())
    assert np.array_equal(t.score, s.score) and t.counter == 1 and np.array_equal(t.assign(20), s.assign(20))
    with pytest.raises(ValueError, match="scenarios"):
        ScenarioSampler(5).load_state_dict(s.state_dict())
    with pytest.raises(ValueError, match="scores"):
        ScenarioSampler(7, mode="abs_adv").load_state_dict(s.state_dict())


# ---------------------------------------------------------------- 3. the options' refusals
@pytest.mark.parametrize("kw, match", [
    (dict(scenario_stats=1), "scenario_stats"),
    (dict(scenario_priority="hardest"), "scenario_priority"),
    (dict(scenario_priority=True), "scenario_priority"),
    (dict(scenario_resample_every=0), "scenario_resample_every"),
    (dict(scenario_resample_every=1.5), "scenario_resample_every"),
    (dict(scenario_resample_every=True), "scenario_resample_every"),
    (dict(scenario_score_alpha=-0.1), "scenario_score_alpha"),
    (dict(scenario_score_alpha=1.5), "scenario_score_alpha"),
    (dict(scenario_score_alpha="0.5"), "scenario_score_alpha"),
    (dict(scenario_score_alpha=float("nan")), "scenario_score_alpha"),
    (dict(scenario_uniform_mix=-1e-9), "scenario_uniform_mix"),
    (dict(scenario_uniform_mix=2), "scenario_uniform_mix"),
    (dict(scenario_temperature=0.0), "scenario_temperature"),
    (dict(scenario_temperature=-1.0), "scenario_temperature"),
    (dict(scenario_temperature=float("inf")), "scenario_temperature"),
    (dict(scenario_temperature=None), "scenario_temperature"),
    (dict(scenario_priority="abs_adv"), "abs_adv"),
])
def test_config_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        ppo.PPOConfig(**kw)


def test_config_accepts_what_the_issue_allows():
    c = ppo.PPOConfig()
    assert (c.scenario_stats, c.scenario_priority, c.scenario_resample_every) == (False, None, 1)
    assert (c.scenario_score_alpha, c.scenario_temperature, c.scenario_uniform_mix) == (0.5, 0.3, 0.25)
    ppo.PPOConfig(scenario_stats=True, scenario_priority="failure", scenario_resample_every=3, scenario_score_alpha=0, scenario_uniform_mix=1)
    ppo.PPOConfig(scenario_priority="abs_adv", gae_lambda=0.95)
    ppo.PPOConfig(scenario_priority="abs_adv", bootstrap_truncated=True)
    ppo.PPOConfig(scenario_stats=True, overlap_allreduce=True)    # (overlap_allreduce is not involved)
    c = ppo.PPOConfig(scenario_priority="abs_adv", gae_lambda=0.9)
    c.gae_lambda = None                                           # a config is mutable: the check runs again where it is used
    with pytest.raises(ValueError, match="abs_adv"):
        ppo.check_scenario_config(c)


class _FakeTrainer(ppo.PPOTrainer):
    """the trainer's scenario set-up on an env stand-in: what it refuses is decided before anything touches the device"""

    def __init__(self, env, cfg):
        self.env, self.cfg, self.ctx, self.device = env, cfg, None, env.device
        self._env_id_base = 0
        self._init_scenarios()


@pytest.mark.parametrize("opt", [dict(scenario_stats=True), dict(scenario_priority="failure")])
@pytest.mark.parametrize("tapes, bank", [(0, None), (1, None), (1, object()), (3, None)])
def test_either_option_needs_a_bank_of_at_least_two_tapes(opt, tapes, bank):
    env = types.SimpleNamespace(N=8, device=torch.device("cpu"), mover_bank=bank,
                                sim=types.SimpleNamespace(movers_tapes=tapes, cfg=types.SimpleNamespace(env_id_base=0)))
    with pytest.raises(ValueError, match="bank of at least 2 tapes"):
        _FakeTrainer(env, ppo.PPOConfig(**opt))


# ---------------------------------------------------------------- 4. the checkpoint's sidecar
def _sidecar_trainer(tmp_path, K=3):
    tr = object.__new__(ppo.PPOTrainer)
    tr.cfg = ppo.PPOConfig(scenario_priority="failure", output_dir=str(tmp_path), policy="mlp64x2")
    tr.ctx = None
    tr.i_so_far, tr.t_so_far = 4, 1234
    tr.scenarios, tr._scen_K = ScenarioSampler(K, seed=5), K
    from navbot_ppo_amd import nets
    tr.actor, tr.critic = nets.make_policy("mlp64x2", 16, 2)
    tr.continue_rollouts, tr._reset_pending = False, False
    return tr


def test_sidecar_round_trip(tmp_path):
    tr = _sidecar_trainer(tmp_path)
    tr.scenarios.observe(_sums(3, [4, 0, 8], [1, 0, 8]))
    tr.scenarios.assign(12)
    tr.scenarios.assign(12)
    pa, pc = tr.save_checkpoint()
    side = ppo.PPOTrainer.sidecar_path("scenarios", pa)
    assert os.path.basename(side) == "scenarios_iter0004_step00001234.pth" and os.path.exists(side)
    fresh = _sidecar_trainer(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fresh.load_checkpoint(pa, pc)
    assert fresh.scenarios.counter == 2
    assert np.array_equal(fresh.scenarios.score, tr.scenarios.score, equal_nan=True) and np.isnan(fresh.scenarios.score[1])
    assert np.array_equal(fresh.scenarios.assign(12), tr.scenarios.assign(12))
    # a missing file: ONE warning line and fresh state
    os.remove(side)
    with pytest.warns(UserWarning, match="scenarios_iter0004_step00001234.pth not found") as rec:
        fresh.load_checkpoint(pa, pc)
    assert len(rec) == 1
    assert fresh.scenarios.counter == 0 and np.isnan(fresh.scenarios.score).all()


def test_options_off_write_no_sidecar(tmp_path):
    tr = _sidecar_trainer(tmp_path)
    tr.cfg, tr.scenarios = ppo.PPOConfig(output_dir=str(tmp_path), policy="mlp64x2"), None
    pa, _ = tr.save_checkpoint()
    assert not os.path.exists(ppo.PPOTrainer.sidecar_path("scenarios", pa))
