"""PPOConfig.scenario_stats / scenario_priority in the trainer: 48 envs (three 16-env workgroups), rollout_len 24, policy mlp64x2,
two epochs per update, GAE(0.95), a bank of three blade tapes, episodes capped at 20 steps (every env ends an episode per rollout)."""
import csv
import os

import numpy as np
import pytest
import torch

import test_gpu_group_sums as GS
from _movers import blade_tape
from _ranks import spawn_ranks
from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavsimError, VecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, T, K, CAP = 48, 24, 3, 20
SPECS = [(5, 3, 0.75), (8, 17, 0.60), (13, 32, 0.90)]
TR = dict(policy="mlp64x2", rollout_len=T, max_episode_steps=CAP, n_updates_per_iteration=2, gae_lambda=0.95, seed=2)
BUFS = ("obs", "act", "logp", "rew", "done", "arrive", "ended", "epret", "eplen", "eppath", "rtg")


def _env(assign="random", n=N, env_id_base=0):
    bank, periods, _ = maps.mover_bank([blade_tape(P, M, radius=r) for P, M, r in SPECS])
    return VecEnv(n, map="stage_1", max_episode_steps=CAP, seed=1, device=DEV, env_id_base=env_id_base,
                  movers=dict(bank=bank, periods=periods, assign=assign))


def _trainer(assign="random", **cfg):
    return ppo.PPOTrainer(_env(assign), ppo.PPOConfig(**{**TR, **cfg}))


def _ids(tr):
    return tr.env.sim.movers_tape_id.cpu().numpy().copy()


def _host_sums(tr, ids, with_adv):
    h = lambda name: getattr(tr, name + "_buf").cpu().numpy()
    adv = tr._gae[0].reshape(T, N).cpu().numpy() if with_adv else None
    return ppo.group_sums_reference(h("ended"), h("arrive"), h("done"), h("eplen"), h("epret"), ids, K, adv=adv)


def _snap(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k + "_buf").clone() for k in BUFS}


def bits(x):
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


# ---------------------------------------------------------------- (a) the trainer follows the host mirror
@pytest.mark.parametrize("mode", ["failure", "abs_adv"])
def test_assignment_follows_the_host_sampler(mode):
    tr = _trainer(scenario_priority=mode)
    host = ppo.ScenarioSampler(K, mode=mode, seed=TR["seed"])
    try:
        seen = [_ids(tr)]
        assert np.array_equal(seen[0], maps.mover_tape_ids(K, N))
        for it in range(3):
            gen = tr.env.sim.generation
            lg = tr.iteration()
            G = _host_sums(tr, seen[-1], mode == "abs_adv")
            host.observe(G)
            want = host.assign(N)
            seen.append(_ids(tr))
            assert np.array_equal(seen[-1], want), (it, seen[-1], want)
            assert tr.env.sim.generation == gen + 1
            np.testing.assert_allclose(tr.scenarios.score, host.score, rtol=1e-12, atol=0)
            assert tr.scenarios.counter == host.counter == it + 1
            rate = G[:, 1] / G[:, 0]
            assert lg["train_scenario_success_min"] == rate.min() and abs(lg["train_scenario_success_mean"] - rate.mean()) < 1e-15
            assert np.array_equal(np.bincount(want, minlength=K), [r["envs"] for r in tr.scenario_rows(G)])
        assert any(not np.array_equal(a, b) for a, b in zip(seen[:-1], seen[1:]))   # the envs did move
        assert all(np.bincount(s, minlength=K).min() >= 1 for s in seen)
    finally:
        tr.env.close()


# ---------------------------------------------------------------- (b) a re-assigned world is the world a fresh handle builds
def test_rollout_after_a_reassignment_is_a_fresh_trainers():
    a = _trainer(scenario_priority="failure")
    try:
        before = _ids(a)
        a.iteration()
        ids = _ids(a)
        assert not np.array_equal(ids, before)
        torch.cuda.synchronize()
        weights, base = a.updater.fp.flat.clone(), a._step_base.clone()
        rng_ctr = a.env.sim.get_state()["rng_ctr"]
        a.rollout()
        got = _snap(a)
    finally:
        a.env.close()
    b = _trainer(assign=ids)      # spawn scans and pre-drawn records of a handle that never held another assignment
    try:
        assert np.array_equal(_ids(b), ids) and b.scenarios is None
        b.updater.fp.flat.copy_(weights)
        b._step_base.copy_(base)
        b.env.sim.set_state(rng_ctr=rng_ctr)    # the envs' own random streams stand where the first trainer's stood
        b.rollout()
        want = _snap(b)
    finally:
        b.env.close()
    ended = got["ended"].bool()
    for k in BUFS:
        if k == "eppath":   # written where an episode ended and nowhere else (include/navsim.h), and the trainer does not zero it between
            assert torch.equal(bits(got[k])[ended], bits(want[k])[ended]), k   # rollouts: elsewhere the first trainer's holds its last rollout's
            continue
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert bool(got["ended"].any()) and bool(got["done"].any())


# ---------------------------------------------------------------- (c) both options off
def test_options_off_nothing_differs():
    tr = _trainer()
    try:
        assert tr.scenarios is None and not hasattr(tr, "_scen_ws")
        gen, ids = tr.env.sim.generation, _ids(tr)
        for _ in range(3):
            lg = tr.iteration()
            assert not [k for k in lg if "scenario" in k]
            assert not [k for k in tr.tb_scalars() if k.startswith("scenarios/")]
            assert tr.env.sim.generation == gen
        assert np.array_equal(_ids(tr), ids)
    finally:
        tr.env.close()


# ---------------------------------------------------------------- (d) the statistics alone
def test_stats_alone_write_the_table_and_move_nothing(tmp_path):
    tr = _trainer(scenario_stats=True, output_dir=str(tmp_path), method_name="m", save_freq=1000, episode_csv_rows=0, tb_episode_rows=0)
    want = []
    try:
        gen, ids = tr.env.sim.generation, _ids(tr)
        for it in range(2):
            lg = tr.iteration()
            G = _host_sums(tr, ids, False)
            want.append(G)
            assert lg["train_scenario_success_min"] == (G[:, 1] / G[:, 0]).min()
            assert tr.tb_scalars()["scenarios/train_success_min"] == lg["train_scenario_success_min"]
            assert tr.env.sim.generation == gen and np.array_equal(_ids(tr), ids)
        assert tr.scenarios.counter == 0
        six = np.sum(want[-1], axis=0)
        assert (lg["episodes"], lg["successes"], lg["collisions"], lg["timeouts"]) == tuple(int(v) for v in six[:4])
    finally:
        tr.env.close()
    with open(os.path.join(str(tmp_path), "m", "logs", "m_train_scenarios.csv")) as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["iteration", "scenario", "envs", "episodes", "success_rate", "collision_rate", "timeout_rate", "score", "weight"]
    assert len(rows) == 2 * K
    score = np.full(K, np.nan)
    for it, G in enumerate(want):
        raw = 1 - G[:, 1] / G[:, 0]
        score = raw if it == 0 else 0.5 * score + 0.5 * raw
        for k in range(K):
            r = rows[it * K + k]
            assert (int(r["iteration"]), int(r["scenario"]), int(r["envs"]), int(r["episodes"])) == (it + 1, k, (ids == k).sum(), G[k, 0])
            assert float(r["success_rate"]) == G[k, 1] / G[k, 0] and float(r["collision_rate"]) == G[k, 2] / G[k, 0]
            assert float(r["timeout_rate"]) == G[k, 3] / G[k, 0]
            assert float(r["score"]) == score[k] and 0 < float(r["weight"]) < 1


# ---------------------------------------------------------------- (e) continue_rollouts: a re-assignment is a change of the world
def test_with_continue_rollouts_a_reassignment_resets():
    tr = _trainer(scenario_priority="failure", scenario_resample_every=2, continue_rollouts=True)
    try:
        did, moved, seam = [], [], []
        for _ in range(4):
            ids, last = _ids(tr), tr.obs_buf[T].clone()
            tr.iteration()
            did.append(tr._did_reset)
            seam.append(torch.equal(tr.obs_buf[0], last))
            moved.append(not np.array_equal(_ids(tr), ids))
    finally:
        tr.env.close()
    assert moved == [False, True, False, True]
    assert did == [True, False, True, False]        # the first rollout, and the one behind the re-assignment
    assert seam == [False, True, False, True]       # where it did not reset, row 0 is the row the last rollout stopped at


# ---------------------------------------------------------------- (f) the checkpoint
def test_load_checkpoint_restores_scores_and_counter(tmp_path):
    kw = dict(scenario_priority="abs_adv", output_dir=str(tmp_path), method_name="m", save_freq=1000, episode_csv_rows=0, tb_episode_rows=0)
    tr = _trainer(**kw)
    try:
        tr.iteration()
        tr.iteration()
        score, counter = tr.scenarios.score.copy(), tr.scenarios.counter
        pa, pc = tr.save_checkpoint()
        nxt = tr.scenarios.assign(N)
    finally:
        tr.env.close()
    assert counter == 2 and np.isfinite(score).all()
    fresh = _trainer(**kw)
    try:
        assert fresh.scenarios.counter == 0
        fresh.load_checkpoint(pa, pc)
        assert fresh.scenarios.counter == 2 and np.array_equal(fresh.scenarios.score, score)
        assert np.array_equal(fresh.scenarios.assign(N), nxt)
    finally:
        fresh.env.close()


# ---------------------------------------------------------------- the refusals that need an env
def test_refused_without_a_bank():
    env = VecEnv(N, map="stage_1", max_episode_steps=CAP, seed=1, device=DEV, movers=blade_tape(5, 3))
    try:
        for opt in (dict(scenario_stats=True), dict(scenario_priority="failure")):
            with pytest.raises(ValueError, match="bank of at least 2 tapes"):
                ppo.PPOTrainer(env, ppo.PPOConfig(**{**TR, **opt}))
        with pytest.raises(NavsimError, match="not a bank"):
            env.assign_scenarios(np.zeros(N, np.int32))
        with pytest.raises(NavsimError, match="no bank"):
            env.sim.set_mover_assignment(np.zeros(N, np.int32))
    finally:
        env.close()
    env = _env()
    try:
        for bad in (np.zeros(N - 1, np.int32), np.full(N, K, np.int32), np.full(N, -1, np.int32), np.zeros(N)):
            with pytest.raises(NavsimError, match="assign_scenarios"):
                env.assign_scenarios(bad)
    finally:
        env.close()


# ---------------------------------------------------------------- (g) the table at an odd shape
def test_stats_table_against_the_mirror_at_an_odd_shape(tmp_path):
    """40 envs (the last rollout workgroup holds 8) and a rollout of 137 rows, which navppo_group_sums cuts into 18 chunks -- two
    waves of its second kernel take two -- the last one a single row: the CSV's figures are the host mirror's of the trainer's own
    buffers"""
    n, t_len = 40, 137
    assert int(lib().navppo_group_sums_ws_bytes(t_len, n, K)) // (7 * n * 8) == 18
    env = _env(n=n)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(**{**TR, "rollout_len": t_len}, scenario_stats=True, output_dir=str(tmp_path), method_name="m",
                                           save_freq=1000, episode_csv_rows=0, tb_episode_rows=0))
    try:
        ids = _ids(tr)
        lg = tr.iteration()
        h = {k: getattr(tr, k + "_buf").cpu().numpy() for k in ("ended", "arrive", "done", "eplen", "epret")}
        assert tr._scen_ws.numel() == 18 * 7 * n * 8
    finally:
        env.close()
    G = ppo.group_sums_reference(h["ended"], h["arrive"], h["done"], h["eplen"], h["epret"], ids, K)
    assert (G[:, 0] > 0).all() and G[:, 7].sum() == t_len * n and np.array_equal(G[:, 7], t_len * np.bincount(ids, minlength=K))
    assert (lg["episodes"], lg["successes"], lg["collisions"], lg["timeouts"]) == tuple(int(v) for v in G[:, :4].sum(axis=0))
    assert lg["train_scenario_success_min"] == (G[:, 1] / G[:, 0]).min()
    with open(os.path.join(str(tmp_path), "m", "logs", "m_train_scenarios.csv")) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == K
    host = ppo.ScenarioSampler(K, seed=TR["seed"])
    host.observe(G)
    for k, r in enumerate(rows):
        assert (int(r["iteration"]), int(r["scenario"]), int(r["envs"]), int(r["episodes"])) == (1, k, (ids == k).sum(), G[k, 0])
        assert float(r["success_rate"]) == G[k, 1] / G[k, 0] and float(r["collision_rate"]) == G[k, 2] / G[k, 0]
        assert float(r["timeout_rate"]) == G[k, 3] / G[k, 0] and float(r["score"]) == host.score[k]


# ---------------------------------------------------------------- (h) two ranks
ROLLOUT = ("ended", "arrive", "done", "eplen", "epret")


def _scen_rank_worker(rank, world, port, path, mode):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduce here
    ctx = ppo.DistCtx(device="cuda:0")
    lo, hi = ctx.shard(N)
    env = _env(n=hi - lo, env_id_base=lo)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(**TR, scenario_priority=mode), ctx)
    tables, its = [], []
    step = tr._scenario_step

    def recording_step(G):      # the global table, as the iteration read it back behind its one all-reduce
        tables.append(np.array(G, dtype=np.float64).reshape(K, 8))
        return step(G)

    tr._scenario_step = recording_step
    try:
        first = _ids(tr)
        for _ in range(2):
            ids = _ids(tr)
            tr.iteration()
            torch.cuda.synchronize()
            it = {k: getattr(tr, k + "_buf").cpu().numpy() for k in ROLLOUT}
            it.update(ids=ids, adv=tr._gae[0].reshape(T, hi - lo).cpu().numpy() if mode == "abs_adv" else None, after=_ids(tr),
                      host=np.array(tr._scen_ids_host), score=tr.scenarios.score.copy(), counter=tr.scenarios.counter)
            its.append(it)
        torch.save(dict(first=first, its=its, tables=tables, base=tr._env_id_base, flat=tr.updater.fp.flat.cpu()), f"{path}.{rank}")
    finally:
        env.close()
    ctx.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("mode", ["failure", "abs_adv"])
def test_two_ranks_equal_one_process_that_plays_both(tmp_path, mode):
    """Shards of 24 + 24 envs: the ranks hold one score, one counter and one global assignment, each rank's device ids are its
    slice of it, and the table behind the all-reduce is the host mirror's over both ranks' buffers side by side.  The single run of
    48 envs starts from the same weights, so its first rollout, its first table's counts and its first re-assignment are the same."""
    path = str(tmp_path / "scen")
    spawn_ranks(_scen_rank_worker, 2, lambda port: (2, port, path, mode))
    ranks = [torch.load(f"{path}.{r}", weights_only=False) for r in range(2)]
    half = N // 2
    assert [r["base"] for r in ranks] == [0, half] and torch.equal(ranks[0]["flat"], ranks[1]["flat"])
    assert np.array_equal(np.concatenate([r["first"] for r in ranks]), maps.mover_tape_ids(K, N))
    with_adv = mode == "abs_adv"
    for it in range(2):
        a, b = (r["its"][it] for r in ranks)
        assert np.array_equal(a["score"], b["score"]) and a["counter"] == b["counter"] == it + 1
        assert np.array_equal(a["host"], b["host"]) and a["host"].shape == (N,)
        assert np.array_equal(a["after"], a["host"][:half]) and np.array_equal(b["after"], a["host"][half:])
        assert np.array_equal(np.bincount(a["host"], minlength=K) >= 1, [True] * K)
        h = {k: np.concatenate([a[k], b[k]], axis=1) for k in ROLLOUT}
        ids = np.concatenate([a["ids"], b["ids"]])
        adv = np.concatenate([a["adv"], b["adv"]], axis=1) if with_adv else None
        want = ppo.group_sums_reference(h["ended"], h["arrive"], h["done"], h["eplen"], h["epret"], ids, K, adv=adv)
        bounds = GS._bounds(dict(ended=h["ended"], ep_return=h["epret"], adv=adv, group=ids), K, with_adv)
        for r in ranks:
            GS._assert_sums(r["tables"][it], want, bounds, f"{mode}, iteration {it + 1}, rank {r['base'] // half}")
        assert np.array_equal(ranks[0]["tables"][it].view(np.int64), ranks[1]["tables"][it].view(np.int64))
        assert (want[:, 0] > 0).all() and with_adv == bool(want[:, 6].any())
    assert not np.array_equal(ranks[0]["its"][0]["host"], maps.mover_tape_ids(K, N))      # the envs did move
    # the single run
    tr = _trainer(scenario_priority=mode)
    try:
        assert np.array_equal(_ids(tr), maps.mover_tape_ids(K, N))
        tr.iteration()
        G = _host_sums(tr, maps.mover_tape_ids(K, N), with_adv)
        exact = [0, 1, 2, 3, 4, 7]
        assert np.array_equal(ranks[0]["tables"][0][:, exact], G[:, exact])
        if mode == "failure":     # the score reads the counts alone
            assert np.array_equal(tr.scenarios.score, ranks[0]["its"][0]["score"])
        else:
            np.testing.assert_allclose(tr.scenarios.score, ranks[0]["its"][0]["score"], rtol=1e-12, atol=0)
        assert np.array_equal(_ids(tr), ranks[0]["its"][0]["host"])
    finally:
        tr.env.close()
