#!/usr/bin/env python3
"""Dev tool: the first learning record with movers, recorded and not gated (authored scenes, three seeds: a record, not a claim).
mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes), gae_lambda=0.95, norm_reward=True, max_grad_norm=0.5, everything else
the defaults.  Training scenes: (a) "orbit4" -- one choreography, phase-shifted over the envs; (b) "random:32" seed 0 -- a bank of 32
scenarios, one per env (navsim_set_mover_bank).  After `iterations` iterations each actor is evaluated deterministically (one
persistent launch, 1024 episodes, arrival threshold 0.4) on three sets: "orbit4"; the held-out bank "random:32" seed 1; and the
stage_2 map without movers (stage_1 plus four fixed pillars: the transfer a clutter-trained policy should make).  The result is a
2 x 3 table of success rates, the per-scenario minimum beside the mean where the set is a bank.
usage: python tools/learning_ab_movers.py [iterations=60] [--seeds 3] [--out profiles/mover_bank_learning.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mover_bank_learning.txt"))
args = ap.parse_args()
N, T = 4096, 512
TRAIN = [("orbit4", "orbit4"), ("random:32 seed 0", dict(name="random:32", seed=0))]
EVAL = [("orbit4", dict(map="stage_1", movers="orbit4")), ("random:32 seed 1 (held out)", dict(map="stage_1", movers=dict(name="random:32", seed=1))),
        ("stage_2, no movers", dict(map="stage_2", movers=None))]
lines = [f"# learning record with movers (tools/learning_ab_movers.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, "
         f"{N} envs x {T} steps, {args.iterations} iterations, gae_lambda 0.95, norm_reward, max_grad_norm 0.5; deterministic evaluation of "
         f"{args.episodes} episodes per set at the end", "# authored scenes: parity unpinned (no reference geometry); three seeds: a record, not a claim"]
table = {}
for tname, movers in TRAIN:
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed, movers=movers)
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=0.95))
        lines.append(f"trained on {tname}, seed {seed}:")
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            if it % 10 == 0 or it == 1:
                lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  coll {lg['collisions'] / max(lg['episodes'], 1):.4f}  "
                             f"tmo {lg['timeouts'] / max(lg['episodes'], 1):.4f}  ret {lg['avg_ep_rews']:8.2f}")
        for ename, world in EVAL:
            s = ev.evaluate(tr.actor, num_episodes=args.episodes, max_timesteps_per_episode=500, n_parallel=1024, seed=1000 + seed,
                            device=env.device, persistent=True, log=None, **world)
            mn = s.get("scenario_success_min")
            table.setdefault((tname, ename), []).append((s["success_rate"], mn))
            lines.append(f"  eval on {ename}: success {s['success_rate']:.4f} collision {s['collision_rate']:.4f} timeout {s['timeout_rate']:.4f}"
                         + (f"  per-scenario success min {mn:.4f} mean {s['scenario_success_mean']:.4f}" if mn is not None else ""))
        print(lines[-1], tname, seed, flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
lines.append("# success rate after training, mean over the seeds (per seed) [per-scenario minimum, mean over the seeds]")
for tname, _ in TRAIN:
    for ename, _ in EVAL:
        rows = table[(tname, ename)]
        mins = [m for _, m in rows if m is not None]
        lines.append(f"# trained on {tname:<17s} evaluated on {ename:<28s}: {sum(a for a, _ in rows) / len(rows):.4f} ("
                     + ", ".join(f"{a:.4f}" for a, _ in rows) + ")" + (f" [{sum(mins) / len(mins):.4f}]" if mins else ""))
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-7:]))
