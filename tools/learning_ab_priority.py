#!/usr/bin/env python3
"""Dev tool: the learning record of scenario-prioritised training, recorded and not gated (authored scenes, three seeds: a record, not
a claim).  The configuration of tools/learning_ab_movers.py: mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes),
gae_lambda=0.95, norm_reward=True, max_grad_norm=0.5, trained on the bank "random:32" seed 0.  Legs: uniform (every env keeps the
scenario the hash gave it; scenario_stats on, which moves nothing), scenario_priority="failure", scenario_priority="abs_adv".  After
`iterations` iterations each actor is evaluated deterministically (one persistent launch, 1024 episodes, arrival threshold 0.4) on the
held-out bank "random:32" seed 1: mean and worst scenario; the worst TRAINING scenario of the last iteration (noisy rollouts) and the
envs the worst-scoring scenario ended with are recorded beside them.
usage: python tools/learning_ab_priority.py [iterations=60] [--seeds 3] [--out profiles/scenario_priority_learning.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scenario_priority_learning.txt"))
args = ap.parse_args()
N, T = 4096, 512
LEGS = [("uniform", dict(scenario_stats=True)), ("failure", dict(scenario_priority="failure")), ("abs_adv", dict(scenario_priority="abs_adv"))]
HELD_OUT = dict(map="stage_1", movers=dict(name="random:32", seed=1))
lines = [f"# learning record of scenario priority (tools/learning_ab_priority.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): "
         f"mlp64x2, {N} envs x {T} steps, {args.iterations} iterations, gae_lambda 0.95, norm_reward, max_grad_norm 0.5, trained on random:32 seed 0; "
         f"deterministic evaluation of {args.episodes} episodes on the held-out random:32 seed 1 at the end",
         "# authored scenes: parity unpinned (no reference geometry); three seeds: a record, not a claim"]
table = {}
for leg, opts in LEGS:
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed, movers=dict(name="random:32", seed=0))
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=0.95, **opts))
        lines.append(f"{leg}, seed {seed}:")
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            if it % 10 == 0 or it == 1:
                lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  coll {lg['collisions'] / max(lg['episodes'], 1):.4f}  "
                             f"tmo {lg['timeouts'] / max(lg['episodes'], 1):.4f}  train scenarios min {lg['train_scenario_success_min']:.4f} "
                             f"mean {lg['train_scenario_success_mean']:.4f}  envs per scenario min {min(r['envs'] for r in tr.scenario_table)} "
                             f"max {max(r['envs'] for r in tr.scenario_table)}")
        worst = min(tr.scenario_table, key=lambda r: r["success_rate"])
        s = ev.evaluate(tr.actor, num_episodes=args.episodes, max_timesteps_per_episode=500, n_parallel=1024, seed=1000 + seed,
                        device=env.device, persistent=True, log=None, **HELD_OUT)
        table.setdefault(leg, []).append((s["success_rate"], s["scenario_success_min"], lg["train_scenario_success_min"]))
        lines.append(f"  held out: success {s['success_rate']:.4f} collision {s['collision_rate']:.4f} timeout {s['timeout_rate']:.4f}  per-scenario "
                     f"success min {s['scenario_success_min']:.4f} mean {s['scenario_success_mean']:.4f};  worst training scenario "
                     f"{worst['scenario']}: success {worst['success_rate']:.4f} on {worst['envs']} envs ({worst['episodes']} episodes)")
        print(lines[-1], leg, seed, flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
lines.append("# mean over the seeds (per seed): held-out success | held-out worst scenario | worst training scenario of the last iteration")
for leg, _ in LEGS:
    rows = table[leg]
    cell = lambda j: f"{sum(r[j] for r in rows) / len(rows):.4f} (" + ", ".join(f"{r[j]:.4f}" for r in rows) + ")"
    lines.append(f"# {leg:<8s}: {cell(0)} | {cell(1)} | {cell(2)}")
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-4:]))
