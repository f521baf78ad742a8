#!/usr/bin/env python3
"""Dev tool: does the policy learn more among moving obstacles when it sees the last three scans?  Recorded and not gated (authored
scenes, three seeds: a record, not a claim -- "no difference" is a result).  The configuration of tools/learning_ab_movers.py:
mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes), gae_lambda=0.95, norm_reward=True, max_grad_norm=0.5, everything else
the defaults; trained on the bank "random:32" seed 0 (one scenario per env) with PPOConfig.scan_history off and on.  After
`iterations` iterations each actor is evaluated deterministically (one persistent launch, 1024 episodes, arrival threshold 0.4) on
the held-out bank "random:32" seed 1: mean success and the per-scenario minimum.
usage: python tools/learning_ab_history.py [iterations=60] [--seeds 3] [--out profiles/scan_history_learning.txt]"""
import argparse
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import evaluate as ev
from navbot_ppo_amd import ppo
from navbot_ppo_amd.env import VecEnv

ap = argparse.ArgumentParser()
ap.add_argument("iterations", type=int, nargs="?", default=60)
ap.add_argument("--seeds", type=int, default=3)
ap.add_argument("--episodes", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_history_learning.txt"))
args = ap.parse_args()
N, T = 4096, 512
TRAIN = dict(name="random:32", seed=0)
HELD_OUT = dict(name="random:32", seed=1)
lines = [f"# learning record with scan history (tools/learning_ab_history.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): "
         f"mlp64x2, {N} envs x {T} steps, {args.iterations} iterations, gae_lambda 0.95, norm_reward, max_grad_norm 0.5, trained on random:32 "
         f"seed 0; deterministic evaluation of {args.episodes} episodes on random:32 seed 1 (held out) at the end",
         "# authored scenes: parity unpinned (no reference geometry); three seeds: a record, not a claim"]
table = {}
for history in (False, True):
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed, movers=TRAIN)
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=0.95,
                                               scan_history=history))
        lines.append(f"scan_history={history}, seed {seed}:")
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            if it % 10 == 0 or it == 1:
                lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  coll {lg['collisions'] / max(lg['episodes'], 1):.4f}  "
                             f"tmo {lg['timeouts'] / max(lg['episodes'], 1):.4f}  ret {lg['avg_ep_rews']:8.2f}  iter {lg['iter_time'] * 1e3:6.1f} ms")
        s = ev.evaluate(tr.actor, num_episodes=args.episodes, max_timesteps_per_episode=500, n_parallel=1024, seed=1000 + seed,
                        device=env.device, persistent=True, log=None, map="stage_1", movers=HELD_OUT)
        table.setdefault(history, []).append((s["success_rate"], s["scenario_success_min"]))
        lines.append(f"  eval on random:32 seed 1 (held out): success {s['success_rate']:.4f} collision {s['collision_rate']:.4f} "
                     f"timeout {s['timeout_rate']:.4f}  per-scenario success min {s['scenario_success_min']:.4f} mean {s['scenario_success_mean']:.4f}")
        print(lines[-1], history, seed, flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
lines.append("# held-out success after training, mean over the seeds (per seed) [per-scenario minimum, mean over the seeds (per seed)]")
for history in (False, True):
    rows = table[history]
    lines.append(f"# scan_history={str(history):<5s}: {sum(a for a, _ in rows) / len(rows):.4f} (" + ", ".join(f"{a:.4f}" for a, _ in rows) + ")"
                 f" [{sum(m for _, m in rows) / len(rows):.4f} (" + ", ".join(f"{m:.4f}" for _, m in rows) + ")]")
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-3:]))
