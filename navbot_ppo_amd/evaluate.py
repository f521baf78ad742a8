"""Evaluation mode: the reference's ``main.evaluate`` (project_ppo/src/main.py:135-252) on the batched simulator.

Loads the newest ``actor_iter*_step*.pth`` (or an explicit path), runs ``num_episodes`` episodes with the
DETERMINISTIC mean action (no sampling, main.py:197-199) and the evaluation arrival threshold 0.4
(``is_training=False``, environment_new.py:44-47), and writes the reference's per-episode CSV
``<output_dir>/<method>/logs/<method>_eval_episodes.csv`` with its columns
``episode,success,collision,timeout,length,return,path_length,time`` (main.py:179) plus the summary it prints
(main.py:236-250).  Episodes run ``n_parallel`` at a time; each env plays a fixed quota of whole episodes back to back; the
``time`` column is the episode's share of the wall clock (length x mean step time).

(The reference's own loop crashes on its first step -- it feeds a (1,2) action so ``action[1]`` raises, SURVEY A3#8;
this implements the intended behaviour.)
"""
import csv
import glob
import os
import time

import numpy as np
import torch

from . import nets
from .env import VecEnv


def find_latest_checkpoint(output_dir, method_name, prefix="actor"):
    d = os.path.join(output_dir, method_name, "checkpoints")
    paths = sorted(glob.glob(os.path.join(d, f"{prefix}_iter*_step*.pth"))) or sorted(glob.glob(os.path.join(d, f"{prefix}_step*.pth")))
    return paths[-1] if paths else None


def load_actor(path, device):
    sd = torch.load(path, map_location="cpu")
    policy = "resmlp512" if any(k.startswith("rb1.") for k in sd) else "mlp64x2"
    in_dim = (sd["rb1.fc1.weight"] if policy == "resmlp512" else sd["layer1.weight"]).shape[1]  # main.py:66-75
    actor, _ = nets.make_policy(policy, in_dim, 2)
    actor.load_state_dict(sd)
    return actor.to(device).eval(), policy


def reads_scan_history(actor, n_beams=10):
    """True for a 42-input mlp64x2 actor on a 10-beam env: a checkpoint trained with PPOConfig.scan_history, whose rows are the
    scan-history rows of env.stack_rows_reference (on 36 beams the same width is the ordinary row)."""
    return isinstance(actor, nets.MLP64Actor) and actor.layer1.weight.shape[1] == 42 and n_beams == 10


def persistent_policy(actor, n_beams=10):
    """(policy name, flat float32 actor in the layout of include/navppo.h) for VecEnv.evaluate_policy; ValueError if the actor
    or the beam count has no evaluation kernel -- ``evaluate(persistent=True)`` never falls back to the stepping loop."""
    if isinstance(actor, nets.MLP64Actor):
        policy, beams = "mlp64x2", (10, 36)
    elif isinstance(actor, nets.ResMLPActor):
        policy, beams = "resmlp512", (10,)
    else:
        raise ValueError(f"evaluate(persistent=True): no evaluation kernel for an actor of type {type(actor).__name__} "
                         "(navsim_evaluate_mlp64 runs nets.MLP64Actor, navsim_evaluate_resmlp512 nets.ResMLPActor)")
    in_dim = (actor.rb1.fc1.weight if policy == "resmlp512" else actor.layer1.weight).shape[1]
    if reads_scan_history(actor, n_beams):   # navsim_evaluate_mlp64_hist: the 42-64-64 actor on 10 beams
        return policy, nets.flat_actor_params(actor)
    if n_beams not in beams or in_dim != n_beams + 6:
        raise ValueError(f"evaluate(persistent=True): no evaluation kernel for policy {policy} with {in_dim}-wide observations on "
                         f"{n_beams} beams (instantiated for {' / '.join(str(b) for b in beams)} beams)")
    return policy, nets.flat_actor_params(actor)


@torch.no_grad()
def evaluate(actor, num_episodes=100, max_timesteps_per_episode=500, map="stage_1", n_parallel=None, seed=0, device=None,
             output_dir="", method_name="baseline", log=print, persistent=False, timing=None, movers=None, scan_pool=1):
    """Every env plays a FIXED quota of q = ceil(num_episodes / n_parallel) whole episodes (its first q; later ones are
    ignored) and stepping continues until every env has met it, so which episodes are reported does not depend on how
    long they last -- taking "the first num_episodes to finish" would over-sample short episodes (early collisions) and
    under-report timeouts.  Rows are ordered episode-slot-major (slot 0 of every env, then slot 1, ...) and cut to
    num_episodes.  Everything stays on the device; the host looks at a counter every 16 steps.

    persistent=True replaces the stepping loop by ONE launch (VecEnv.evaluate_policy: the HIP actor and the env step alternate
    inside the kernel, the quota is kept on chip, a workgroup stops when its envs are done); rows, order, CSV, summary and log
    line come from the same code.  The ``time`` column is then length x (wall clock / the most steps any workgroup ran).  An
    actor or beam count without an evaluation kernel raises ValueError.  movers: moving obstacles as for VecEnv; with a bank of
    tapes the result also holds ``scenarios`` (scenario_report: per tape id episodes and success / collision / time-out rate),
    ``scenario_success_min`` / ``_mean``, logged and, with an output_dir, written to ``<method>_eval_scenarios.csv``.  timing: a dict that receives ``seconds`` (wall clock
    of the stepping alone) and ``steps`` (env steps behind it).  scan_pool: sector LiDAR as for VecEnv (the sensor world the policy is
    judged in; a harder one than scan_pool=1 -- it detects the collisions with obstacles the 10 beams pass by)."""
    n_par = int(n_parallel or min(num_episodes, 1024))
    quota = -(-int(num_episodes) // n_par)
    history = reads_scan_history(actor)   # a scan_history checkpoint: both forms feed it the history rows (the env has 10 beams)
    if persistent:
        policy, flat_actor = persistent_policy(actor)
    env = VecEnv(n_par, map=map, max_episode_steps=max_timesteps_per_episode, auto_reset=True, is_training=False, seed=seed,
                 device=device, movers=movers, scan_pool=scan_pool)
    dev = env.device
    # a bank of tapes (one scenario per env): the episode table is also grouped by the env's tape id, on the host
    tape_id = None if env.sim.movers_tape_id is None else env.sim.movers_tape_id.cpu().numpy()
    n_tapes = env.sim.movers_tapes
    if persistent:
        flat_actor = flat_actor.to(dev)
        torch.cuda.synchronize(dev)
        t0 = time.time()
        tab = env.evaluate_policy(flat_actor, quota, policy=policy, history=history)
        torch.cuda.synchronize(dev)
        seconds = time.time() - t0
        if int(tab.count.min()) < quota:
            raise RuntimeError("evaluate(persistent=True): an env did not finish its quota of episodes")
        steps = int(tab.steps.max())
        env.close()
        fl = tab.flags
        res = torch.stack([(fl & 1).double(), ((fl >> 1) & 1).double(), ((fl >> 2) & 1).double(), tab.length.double(),
                           tab.ret.double(), tab.path.double()], 2)
        return _report(res, quota, n_par, num_episodes, seconds, steps, output_dir, method_name, log, timing, tape_id, n_tapes)
    actor = actor.to(dev).eval()
    obs = env.reset()
    window = None
    if history:
        from .env import HistoryWindow
        window = HistoryWindow(n_par, dev, obs.dtype)
        obs = window.reset(obs)
    count = torch.zeros(n_par, dtype=torch.int64, device=dev)
    res = torch.zeros((quota, n_par, 6), dtype=torch.float64, device=dev)   # success, collision, timeout, length, return, path
    env_ids = torch.arange(n_par, device=dev)
    t0, steps = time.time(), 0
    max_steps = quota * max_timesteps_per_episode + 1
    while steps < max_steps:
        action = actor(obs.float())                                   # deterministic mean action, main.py:197-199
        obs, rew, done, arrive = env.step(action)
        io = env.io
        if window is not None:
            obs = window.push(obs, io.ended)
        take = io.ended.bool() & (count < quota)
        a, d = arrive.bool(), done.bool()
        ln = io.ep_length.double()
        row = torch.stack([a.double(), (d & ~a).double(),
                           (~d & ~a & (io.ep_length >= max_timesteps_per_episode)).double(),      # main.py:214-216
                           ln, io.ep_return.double(), io.ep_path.double()], 1)                    # path: main.py:200-204
        slot = torch.clamp(count, max=quota - 1)
        cur = res[slot, env_ids]
        res[slot, env_ids] = torch.where(take[:, None], row, cur)
        count += take.long()
        steps += 1
        if steps % 16 == 0 and bool((count >= quota).all()):
            break
    torch.cuda.synchronize(dev)
    seconds = time.time() - t0
    env.close()
    return _report(res, quota, n_par, num_episodes, seconds, steps, output_dir, method_name, log, timing, tape_id, n_tapes)


def make_eval_env(train_env, cfg, device):
    """The evaluation envs of PPOConfig.eval_every: the training env's world (VecEnv.world_args; movers: cfg.eval_movers if set),
    min(eval_episodes, 1024) envs with the evaluation arrival threshold and a goal / spawn stream of their own."""
    w = dict(getattr(train_env, "world_args", None) or {})   # (any env with N, B, D and a sim can train; only a VecEnv says this)
    if not w:
        raise ValueError("PPOConfig.eval_every: the training env does not describe its world (VecEnv.world_args)")
    if torch.is_tensor(w["map"]) and w["map"].dim() == 3:
        raise ValueError("PPOConfig.eval_every: a per-env segment tensor cannot be reused for the evaluation envs; pass a map "
                         "name or a shared [S, 4] map (per_env_map=True replicates it)")
    n_par = min(int(cfg.eval_episodes), 1024)
    if n_par < 1:
        raise ValueError("PPOConfig.eval_episodes must be at least 1")
    seed = (int(cfg.seed) * 1000003 + 7919) & 0xFFFFFFFF   # its own goal / spawn stream, derived from cfg.seed
    if cfg.eval_movers is not None:   # the held-out set: resolved like VecEnv's movers, given to the evaluation env only
        w["movers"] = cfg.eval_movers
    return VecEnv(n_par, max_episode_steps=cfg.max_episode_steps, auto_reset=True, is_training=False, seed=seed, device=device, **w)


def evaluate_params(env, flat_params, policy, history, eval_episodes):
    """eval_episodes episodes of the actor in the flat parameter buffer in ONE launch on env: the deterministic mean action, a fixed
    quota of whole episodes per env, rows cut slot-major to eval_episodes as evaluate() does.  The sums are taken on the device and
    read with one synchronisation.  Returns the eval_* figures of PPOTrainer.evaluate_now."""
    n_ep = int(eval_episodes)
    quota = -(-n_ep // env.N)
    t0 = time.time()
    tab = env.evaluate_policy(flat_params, quota, policy=policy, history=history)
    cut = lambda x: x.reshape(-1)[:n_ep]
    fl = cut(tab.flags)
    sums = torch.stack([(fl & 1).sum().double(), ((fl >> 1) & 1).sum().double(), ((fl >> 2) & 1).sum().double(),
                        cut(tab.length).double().sum(), cut(tab.ret).double().sum(), cut(tab.path).double().sum(),
                        tab.count.min().double(), tab.steps.max().double()])
    n_tapes = env.sim.movers_tapes if env.sim.movers_tape_id is not None else 0
    if n_tapes:   # a bank of tapes: episodes and successes per scenario (row r of the table was played by env r mod N)
        ids = cut(env.sim.movers_tape_id.long().repeat(quota))
        sums = torch.cat([sums, torch.bincount(ids, minlength=n_tapes).double(),
                          torch.bincount(ids, weights=(fl & 1).double(), minlength=n_tapes)])
    sums = sums.cpu().numpy()   # the one host sync
    per_tape = sums[8:].reshape(2, -1)
    if int(sums[6]) < quota:
        raise RuntimeError("evaluate_now: an env did not finish its quota of episodes")
    sums = [float(v) for v in sums]
    out = dict(eval_episodes=n_ep, eval_success=sums[0] / n_ep, eval_collision=sums[1] / n_ep, eval_timeout=sums[2] / n_ep,
               eval_length=sums[3] / n_ep, eval_return=sums[4] / n_ep, eval_path_length=sums[5] / n_ep,
               eval_steps=int(sums[7]), eval_time=time.time() - t0)
    if n_tapes:
        rate = per_tape[1][per_tape[0] > 0] / per_tape[0][per_tape[0] > 0]   # (scenarios that played at least one episode)
        out.update(eval_scenario_success_min=float(rate.min()), eval_scenario_success_mean=float(rate.mean()))
    return out


def scenario_report(rows, tape_id, n_tapes):
    """The episode table grouped by scenario: rows = evaluate()'s rows in their slot-major order (row r was played by env
    r mod len(tape_id)), tape_id [n_par] the tape of each env -> one dict per tape of the bank: scenario, episodes and the success,
    collision and time-out rate of its episodes (NaN for a scenario no reported episode played)."""
    tape_id = np.asarray(tape_id).reshape(-1)
    arr = np.array([r[1:4] for r in rows], dtype=np.float64).reshape(-1, 3)
    of_row = tape_id[np.arange(arr.shape[0]) % tape_id.size]
    out = []
    for k in range(int(n_tapes)):
        sel = arr[of_row == k]
        rate = sel.mean(axis=0) if sel.shape[0] else np.full(3, np.nan)
        out.append(dict(scenario=k, episodes=int(sel.shape[0]), success_rate=float(rate[0]), collision_rate=float(rate[1]),
                        timeout_rate=float(rate[2])))
    return out


def scenario_success(scenarios):
    """(min, mean) of the success rate over the scenarios that played at least one episode"""
    s = [d["success_rate"] for d in scenarios if d["episodes"] > 0]
    return (min(s), sum(s) / len(s)) if s else (float("nan"), float("nan"))


def _report(res, quota, n_par, num_episodes, seconds, steps, output_dir, method_name, log, timing, tape_id=None, n_tapes=0):
    """rows, CSV, summary and log line of evaluate() from the [quota, n_par, 6] episode table of either stepping path"""
    sec_per_step = seconds / max(steps, 1)
    if timing is not None:
        timing.update(seconds=seconds, steps=steps)
    flat = res.reshape(quota * n_par, 6)[:num_episodes].cpu().numpy()
    rows = [[k, int(r[0]), int(r[1]), int(r[2]), int(r[3]), float(r[4]), float(r[5]), float(r[3]) * sec_per_step]
            for k, r in enumerate(flat)]
    arr = np.array([r[1:] for r in rows], dtype=np.float64)
    summary = dict(episodes=len(rows), success_rate=arr[:, 0].mean(), collision_rate=arr[:, 1].mean(), timeout_rate=arr[:, 2].mean(),
                   mean_length=arr[:, 3].mean(), std_length=arr[:, 3].std(), mean_return=arr[:, 4].mean(), std_return=arr[:, 4].std(),
                   mean_path_length=arr[:, 5].mean())
    csv_path = None
    if output_dir:
        log_dir = os.path.join(output_dir, method_name, "logs")
        os.makedirs(log_dir, exist_ok=True)
        csv_path = os.path.join(log_dir, f"{method_name}_eval_episodes.csv")
        with open(csv_path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["episode", "success", "collision", "timeout", "length", "return", "path_length", "time"])  # main.py:179
            w.writerows(rows)
    if log:
        log(f"EVALUATION SUMMARY  method={method_name} episodes={len(rows)} success={summary['success_rate'] * 100:.2f}% "
            f"collision={summary['collision_rate'] * 100:.2f}% timeout={summary['timeout_rate'] * 100:.2f}% "
            f"len={summary['mean_length']:.2f}+-{summary['std_length']:.2f} return={summary['mean_return']:.2f}+-{summary['std_return']:.2f}"
            + (f" csv={csv_path}" if csv_path else ""))
    summary["csv"] = csv_path
    summary["rows"] = rows
    if tape_id is not None:
        sc = scenario_report(rows, tape_id, n_tapes)
        summary["scenarios"] = sc
        summary["scenario_success_min"], summary["scenario_success_mean"] = scenario_success(sc)
        summary["scenarios_csv"] = None
        if output_dir:
            summary["scenarios_csv"] = os.path.join(log_dir, f"{method_name}_eval_scenarios.csv")
            with open(summary["scenarios_csv"], "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["scenario", "episodes", "success_rate", "collision_rate", "timeout_rate"])
                w.writerows([[d["scenario"], d["episodes"], d["success_rate"], d["collision_rate"], d["timeout_rate"]] for d in sc])
        if log:
            log(f"EVALUATION SCENARIOS  method={method_name} scenarios={len(sc)} success min={summary['scenario_success_min'] * 100:.2f}% "
                f"mean={summary['scenario_success_mean'] * 100:.2f}%  "
                + " ".join(f"[{d['scenario']}: n={d['episodes']} succ={d['success_rate'] * 100:.1f}% coll={d['collision_rate'] * 100:.1f}% "
                           f"tmo={d['timeout_rate'] * 100:.1f}%]" for d in sc))
    return summary
