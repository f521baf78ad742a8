"""The trainer's host side after its split (no GPU): train_log's CSV helper, scalars, progress line and read-back sections, and the one
sidecar table that save_checkpoint / load_checkpoint walk.  The expected scalars and lines are those PPOTrainer.tb_scalars / learn gave
for the same two dicts before the split."""
import csv
import os
import warnings

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo, train_log
from navbot_ppo_amd.scenarios import ScenarioSampler

CFG = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=6, rollout_len=16)
# one iteration's figures with no option on ...
BASE = dict(iteration=3, t_so_far=12345, avg_ep_rews=-1.5, success_rate=0.25, avg_ep_lens=40.5, actor_loss=0.0123, critic_loss=4.5,
            approx_kl=0.0042, steps_per_sec=123456.7, rollout_time=0.016, update_time=0.25, iter_time=0.266, episodes=8, collisions=2,
            timeouts=4, clip_frac=0.125, actor_grad_norm=0.5, critic_grad_norm=2.0, actor_param_delta=0.001, critic_param_delta=0.002,
            var=0.5)
# ... and with every optional key
FULL = dict(BASE, kl_stop_epoch=3, kl_stopped=1, kl_stop_step=7, lr=4.5e-4, lr_ups=2, lr_downs=1, bootstrapped_frac=0.03125,
            train_scenario_success_min=0.125, train_scenario_success_mean=0.375, eval_success=0.75, eval_collision=0.125,
            eval_timeout=0.125, eval_return=12.25, eval_length=33.5, eval_time=0.0625, eval_scenario_success_min=0.5,
            eval_scenario_success_mean=0.625, reward_scale=0.25, ret_rms_mean=1.5, ret_rms_std=4.0, explained_variance=0.875,
            grad_clip_frac_actor=0.5, grad_clip_frac_critic=1.0, skipped_steps_actor=0, skipped_steps_critic=1)
TB_BASE = {"train/success_rate": 0.25, "train/collision_rate": 0.25, "train/timeout_rate": 0.5, "train/mean_return": -1.5,
           "train/mean_ep_length": 40.5, "train/mean_ep_time": 0.0405, "loss/actor": 0.0123, "loss/critic": 4.5, "train/timesteps": 12345,
           "time/rollout": 0.016, "time/update": 0.25, "time/iteration": 0.266, "perf/steps_per_sec": 123456.7,
           "perf/actor_grad_steps": 6, "perf/critic_grad_steps": 6, "ppo/approx_kl": 0.0042, "ppo/entropy": 2.1447298858494,
           "ppo/clip_frac": 0.125, "ppo/actor_grad_norm": 0.5, "ppo/critic_grad_norm": 2.0, "ppo/actor_param_delta": 0.001,
           "ppo/critic_param_delta": 0.002, "ppo/grad_clip_frac_actor": None, "ppo/grad_clip_frac_critic": None,
           "ppo/skipped_steps_actor": None, "ppo/skipped_steps_critic": None, "ppo/kl_stop_epoch": None, "ppo/kl_stopped": None}
TB_FULL = dict(TB_BASE, **{"ppo/grad_clip_frac_actor": 0.5, "ppo/grad_clip_frac_critic": 1.0, "ppo/skipped_steps_actor": 0,
                           "ppo/skipped_steps_critic": 1, "ppo/kl_stop_epoch": 3, "ppo/kl_stopped": 1, "ppo/kl_stop_step": 7,
                           "ppo/lr": 0.00045, "ppo/lr_ups": 2, "ppo/lr_downs": 1, "ppo/reward_scale": 0.25, "ppo/ret_rms_mean": 1.5,
                           "ppo/ret_rms_std": 4.0, "ppo/explained_variance": 0.875, "ppo/bootstrapped_frac": 0.03125,
                           "scenarios/train_success_min": 0.125, "scenarios/train_success_mean": 0.375, "eval/success_rate": 0.75,
                           "eval/collision_rate": 0.125, "eval/timeout_rate": 0.125, "eval/mean_return": 12.25,
                           "eval/mean_ep_length": 33.5, "time/eval": 0.0625})
LINE_BASE = ("[iter    3] t=     12345 mean_ep_rew=   -1.50 succ=0.250 ep_len=  40.5 a_loss=0.0123 c_loss=4.50 kl=0.0042 steps/s=123457 "
             "(rollout 0.016s update 0.250s)")
LINE_FULL = (LINE_BASE + " kl_stop_epoch=3 kl_stopped=1 kl_stop_step=7 lr=4.500e-04 lr_ups=2 lr_downs=1 bootstrapped_frac=0.0312 "
             "train scenarios: min=0.125 mean=0.375 eval: succ=0.750 coll=0.125 tmo=0.125 ret=12.25 len=33.5 (0.062s) "
             "scenarios: min=0.500 mean=0.625")


def test_append_rows_writes_the_header_once_and_creates_the_directory(tmp_path):
    path = str(tmp_path / "run" / "logs" / "m_train_x.csv")
    for k in range(3):
        assert train_log.append_rows(path, ["a", "b"], [[k, 2 * k], [k, "x,y"]]) == path
    assert train_log.append_rows(path, ["a", "b"], []) == path   # no rows on a file that exists: nothing is added
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [["a", "b"]] + [r for k in range(3) for r in ([str(k), str(2 * k)], [str(k), "x,y"])]
    empty = str(tmp_path / "other" / "e.csv")
    train_log.append_rows(empty, ["a", "b"], [])
    assert open(empty).read().splitlines() == ["a,b"]


@pytest.mark.parametrize("lg, tags, line", [(BASE, TB_BASE, LINE_BASE), (FULL, TB_FULL, LINE_FULL)], ids=["no_option", "every_option"])
def test_scalars_and_progress_line_are_what_the_trainer_gave(lg, tags, line):
    sc = train_log.tb_scalars(lg, CFG)
    assert sc == tags and list(sc) == list(tags)   # values, and the order the TensorBoard records are written in
    assert train_log.progress_line(lg) == line
    tr = ppo.PPOTrainer.__new__(ppo.PPOTrainer)    # the forward: a bare trainer with cfg and logger alone
    tr.cfg, tr.logger = CFG, lg
    assert tr.tb_scalars() == tags


def test_scalars_of_an_empty_logger():
    sc = train_log.tb_scalars({}, CFG)
    assert set(sc) == set(TB_BASE) and sc["ppo/entropy"] == 2.6147335150951356   # (init_var 0.8)
    assert {k for k, v in sc.items() if v is not None} == {"train/collision_rate", "train/timeout_rate", "train/mean_ep_time",
                                                           "perf/actor_grad_steps", "perf/critic_grad_steps", "ppo/entropy"}


K = 3


@pytest.mark.parametrize("names", [("episodes",), ("episodes", "scenarios"), ("episodes", "reward_norm"),
                                   ("episodes", "scenarios", "reward_norm")], ids=lambda n: "+".join(n))
def test_read_back_sections_come_back_under_their_names(names):
    length = dict(episodes=6, scenarios=K * 8, reward_norm=5)
    rng = np.random.default_rng(7)
    parts = [(n, torch.from_numpy(rng.standard_normal(length[n]))) for n in names]
    m, sections = train_log.join_sections(parts)
    assert sections == [(n, length[n]) for n in names] and m.dtype == torch.float64 and m.numel() == sum(length[n] for n in names)
    back = train_log.split_sections(m, sections)
    assert list(back) == list(names)
    if len(names) == 1:   # the six alone: the tensor itself, not concatenated and not read
        assert m is parts[0][1] and back["episodes"] is m
        return
    for n, t in parts:
        assert isinstance(back[n], list) and back[n] == t.tolist()
    # the trainer's order of effects: the summed sections first, the reward-norm figures appended behind the collective
    head, hs = train_log.join_sections(parts[:-1])
    tail = parts[-1][1]
    again = train_log.split_sections(torch.cat([head, tail]), hs + [(names[-1], tail.numel())])
    assert again == back


# ---------------------------------------------------------------- the sidecar table
def _bare(tmp_path, **cfg):
    tr = ppo.PPOTrainer.__new__(ppo.PPOTrainer)
    tr.cfg = ppo.PPOConfig(output_dir=str(tmp_path), method_name="m", policy="mlp64x2", **cfg)
    tr.actor, tr.critic = nets.make_policy("mlp64x2")
    tr.i_so_far, tr.t_so_far = 4, 19876
    return tr


def _lrsched(tmp_path, on):
    tr = _bare(tmp_path, **(dict(lr_schedule="adaptive") if on else {}))
    tr.updater = ppo.PPOUpdater(tr.actor, tr.critic, tr.cfg, None, torch.device("cpu"))
    return tr, (lambda: tr.updater.set_lr(1e-3)), (lambda: tr.updater.lr_value), {"lr": 1e-3}, 3e-4


def _retnorm(tmp_path, on):
    tr = _bare(tmp_path, norm_reward=on)
    if on:
        tr._init_ret_rms("cpu")
    return (tr, (lambda: tr._init_ret_rms("cpu", 12.5, 3456.789, 2097152.0001)), (lambda: tr.ret_rms[:3].tolist()),
            {"mean": 12.5, "var": 3456.789, "count": 2097152.0001}, [0.0, 1.0, 1e-4])


def _scenarios(tmp_path, on):
    tr = _bare(tmp_path)
    if on:
        tr.scenarios, tr._scen_K = ScenarioSampler(K, seed=5), K

    def change():
        tr.scenarios.observe(np.array([[4, 1] + [0] * 6, [0] * 8, [8, 8] + [0] * 6], dtype=np.float64))
        tr.scenarios.assign(12)
    state = lambda: ([None if np.isnan(v) else float(v) for v in tr.scenarios.score], tr.scenarios.counter)
    return tr, change, state, {"score": [0.75, float("nan"), 0.0], "counter": 1, "mode": "failure"}, ([None] * K, 0)


@pytest.mark.parametrize("kind, make", [("lrsched", _lrsched), ("retnorm", _retnorm), ("scenarios", _scenarios)])
def test_sidecar_table_one_path_for_every_kind(tmp_path, kind, make):
    tag = "iter0004_step00019876.pth"
    # option off: two files, and a file of that kind beside them is not even opened
    off = make(tmp_path / "off", False)[0]
    assert [row[0] for row in off._sidecars() if row[1]] == []
    pa, pc = off.save_checkpoint()
    assert sorted(os.listdir(os.path.dirname(pa))) == ["actor_" + tag, "critic_" + tag]
    with open(ppo.PPOTrainer.sidecar_path(kind, pa), "w") as f:
        f.write("not a checkpoint")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off.load_checkpoint(pa, pc)
    # option on: the payload as it always was, a round trip into a fresh trainer, no warning
    on, change, state, payload, fresh_state = make(tmp_path / "on", True)
    assert [row[0] for row in on._sidecars() if row[1]] == [kind]
    change()
    pa, pc = on.save_checkpoint()
    side = ppo.PPOTrainer.sidecar_path(kind, pa)
    assert sorted(os.listdir(os.path.dirname(pa))) == sorted(["actor_" + tag, "critic_" + tag, kind + "_" + tag])
    stored = torch.load(side)
    assert list(stored) == list(payload) and all(stored[k] == v or (k == "score" and np.array_equal(stored[k], v, equal_nan=True))
                                                 for k, v in payload.items())
    fresh, _, fresh_get, _, _ = make(tmp_path / "fresh", True)
    assert fresh_get() == fresh_state
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fresh.load_checkpoint(pa, pc)
    assert fresh_get() == state()
    for k, v in on.actor.state_dict().items():
        assert torch.equal(v, fresh.actor.state_dict()[k])
    # a missing file: exactly ONE warning, one line, and the state of a fresh run
    os.remove(side)
    with pytest.warns(UserWarning, match=kind + "_" + tag + " not found") as rec:
        fresh.load_checkpoint(pa, pc)
    assert len(rec) == 1 and "\n" not in str(rec[0].message)
    assert fresh_get() == fresh_state
