#!/usr/bin/env python3
"""Dev tool: the learning record of the sector LiDAR (scan_pool), recorded and not gated (authored scenes, three seeds: a record, not
a claim).  The configuration of tools/learning_ab_movers.py: mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes),
gae_lambda=0.95, norm_reward=True, max_grad_norm=0.5, trained on the bank "random:32" seed 0.  Legs: scan_pool k = 1 (the
reference's 10 beams) and k = 4 (40 rays pooled to the 10 columns).  After `iterations` iterations each actor is evaluated
deterministically (one persistent launch, 1024 episodes, arrival threshold 0.4) on the held-out bank "random:32" seed 1 in BOTH
sensor worlds: a 2 x 2 table of success, collisions, time-outs and the worst scenario.
The k = 4 world detects collisions the k = 1 world lets through (a 0.3 m pillar between two of the 10 beams is neither seen nor hit
there): only the COLUMNS of the table are comparable like for like -- two policies in the same world -- not its diagonal.
usage: python tools/learning_ab_pool.py [iterations=60] [--seeds 3] [--out profiles/scan_pool_learning.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_pool_learning.txt"))
args = ap.parse_args()
N, T = 4096, 512
POOLS = (1, 4)
lines = [f"# learning record of scan_pool (tools/learning_ab_pool.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, "
         f"{N} envs x {T} steps, {args.iterations} iterations, gae_lambda 0.95, norm_reward, max_grad_norm 0.5, trained on random:32 seed 0; "
         f"deterministic evaluation of {args.episodes} episodes on random:32 seed 1 (held out) in both sensor worlds",
         "# authored scenes: parity unpinned (no reference geometry); three seeds: a record, not a claim",
         "# the k = 4 world detects collisions the k = 1 world lets through: compare within an evaluation world (a column), not across"]
table = {}
for k in POOLS:
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed, movers=dict(name="random:32", seed=0), scan_pool=k)
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=0.95))
        lines.append(f"trained with scan_pool {k}, seed {seed}:")
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            if it % 10 == 0 or it == 1:
                lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  coll {lg['collisions'] / max(lg['episodes'], 1):.4f}  "
                             f"tmo {lg['timeouts'] / max(lg['episodes'], 1):.4f}  ret {lg['avg_ep_rews']:8.2f}")
        for ke in POOLS:
            s = ev.evaluate(tr.actor, num_episodes=args.episodes, max_timesteps_per_episode=500, n_parallel=1024, seed=1000 + seed,
                            device=env.device, persistent=True, log=None, map="stage_1", movers=dict(name="random:32", seed=1), scan_pool=ke)
            table.setdefault((k, ke), []).append((s["success_rate"], s["collision_rate"], s["timeout_rate"], s["scenario_success_min"]))
            lines.append(f"  eval in the scan_pool {ke} world: success {s['success_rate']:.4f} collision {s['collision_rate']:.4f} "
                         f"timeout {s['timeout_rate']:.4f}  per-scenario success min {s['scenario_success_min']:.4f} "
                         f"mean {s['scenario_success_mean']:.4f}")
        print(lines[-1], k, seed, flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
lines.append("# mean over the seeds: success / collision / time-out / worst scenario's success (success per seed)")
for k in POOLS:
    for ke in POOLS:
        rows = table[(k, ke)]
        m = [sum(r[j] for r in rows) / len(rows) for j in range(4)]
        lines.append(f"# trained with scan_pool {k}, evaluated in the scan_pool {ke} world: {m[0]:.4f} / {m[1]:.4f} / {m[2]:.4f} / {m[3]:.4f} ("
                     + ", ".join(f"{r[0]:.4f}" for r in rows) + ")")
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-5:]))
