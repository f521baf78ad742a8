#!/usr/bin/env python3
"""Dev tool: the learning record of the learned exploration variance, recorded and not gated (authored scenes, three seeds: a record,
not a claim).  The configuration of tools/learning_ab_movers.py -- mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes),
gae_lambda=0.95, norm_reward=True, max_grad_norm=0.5 -- trained on the bank "random:32" seed 0.  Legs: the reference's fixed variance
schedule against learn_var with ent_coef 0 and 0.01.  Per leg and seed: the variance and the training success rate per iteration, and
after `iterations` iterations a deterministic evaluation (one persistent launch, 1024 episodes, arrival threshold 0.4) on the held-out
bank "random:32" seed 1 -- its success, collision and time-out rates, the per-scenario mean and the worst scenario.
usage: python tools/learning_ab_var.py [iterations=60] [--seeds 3] [--out profiles/learned_var_learning.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "learned_var_learning.txt"))
args = ap.parse_args()
N, T = 4096, 512
LEGS = [("schedule", {}), ("learn_var ent_coef 0", dict(learn_var=True)), ("learn_var ent_coef 0.01", dict(learn_var=True, ent_coef=0.01))]
HELD_OUT = dict(map="stage_1", movers=dict(name="random:32", seed=1))
lines = [f"# learning record of learn_var (tools/learning_ab_var.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, "
         f"{N} envs x {T} steps, {args.iterations} iterations, trained on random:32 seed 0, gae_lambda 0.95, norm_reward, max_grad_norm 0.5; "
         f"deterministic evaluation of {args.episodes} episodes on random:32 seed 1 (held out) at the end",
         "# authored scenes: parity unpinned (no reference geometry); three seeds: a record, not a claim",
         "# per iteration: var = the variance the NEXT rollout draws with (schedule: this rollout's), succ = training success rate"]
table = {}
for lname, opts in LEGS:
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed, movers=dict(name="random:32", seed=0))
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=0.95, **opts))
        lines.append(f"{lname}, seed {seed}:")
        row = []
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            row.append(f"{it}:{lg['var']:.4f}/{lg['success_rate']:.3f}")
        for k in range(0, len(row), 10):
            lines.append("  var/succ  " + "  ".join(row[k:k + 10]))
        s = ev.evaluate(tr.actor, num_episodes=args.episodes, max_timesteps_per_episode=500, n_parallel=1024, seed=1000 + seed,
                        device=env.device, persistent=True, log=None, **HELD_OUT)
        table.setdefault(lname, []).append((lg["success_rate"], lg["var"], s["success_rate"], s["collision_rate"], s["timeout_rate"],
                                            s["scenario_success_min"]))
        lines.append(f"  final training success {lg['success_rate']:.4f} var {lg['var']:.4f}; held out: success {s['success_rate']:.4f} "
                     f"collision {s['collision_rate']:.4f} timeout {s['timeout_rate']:.4f}  per-scenario success min "
                     f"{s['scenario_success_min']:.4f} mean {s['scenario_success_mean']:.4f}")
        print(lname, seed, lines[-1], flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
lines.append("# mean over the seeds (per seed): final training success | final var | held-out success | collision | time-out | worst scenario")
for lname, _ in LEGS:
    rows = table[lname]
    lines.append(f"# {lname:<24s}: " + " | ".join(f"{sum(r[k] for r in rows) / len(rows):.4f} (" + ", ".join(f"{r[k]:.4f}" for r in rows) + ")"
                                                     for k in range(6)))
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-4:]))
