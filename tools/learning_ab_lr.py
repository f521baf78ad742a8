#!/usr/bin/env python3
"""Dev tool: the learning A/B of PPOConfig.lr_schedule="adaptive" against the constant lr = 3e-4, recorded and not gated.  mlp64x2,
4096 envs x 512 steps (stage_1), an rsl_rl-like update: n_updates_per_iteration=5, minibatch_size = a quarter of the batch,
max_grad_norm=0.5, norm_reward=True; seeds 0..2, `iterations` iterations each.  Per iteration: success rate, the learning rate after
the update, its raises / lowerings, the update's mean approx_kl.  The block is appended to profiles/adaptive_lr_epoch.txt behind the
timing block of tools/time_update_lr.py (an earlier A/B block is replaced).
usage: python tools/learning_ab_lr.py [iterations=60] [--out profiles/adaptive_lr_epoch.txt]"""
import argparse
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import ppo
from navbot_ppo_amd.env import VecEnv

ap = argparse.ArgumentParser()
ap.add_argument("iterations", type=int, nargs="?", default=60)
ap.add_argument("--seeds", type=int, default=3)
ap.add_argument("--desired_kl", type=float, default=0.01)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adaptive_lr_epoch.txt"))
args = ap.parse_args()
N, T = 4096, 512
lines = [f"# learning A/B (tools/learning_ab_lr.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, {N} envs x {T} steps, "
         f"{args.iterations} iterations, 5 epochs x 4 minibatches, max_grad_norm 0.5, norm_reward; constant lr 3e-4 against adaptive "
         f"(desired_kl {args.desired_kl})",
         "# per iteration: success rate | lr after the update | raises / lowerings | mean approx_kl of the update's steps"]
final = {}
for sched in (None, "adaptive"):
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed)
        cfg = ppo.PPOConfig(policy="mlp64x2", seed=seed, n_updates_per_iteration=5, minibatch_size=N * T // 4, max_grad_norm=0.5,
                            norm_reward=True, lr_schedule=sched, desired_kl=args.desired_kl)
        tr = ppo.PPOTrainer(env, cfg)
        name = f"{'adaptive' if sched else 'constant'} seed {seed}"
        lines.append(f"{name}:")
        succ = []
        for it in range(1, args.iterations + 1):
            lg = tr.iteration()
            succ.append(lg["success_rate"])
            lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  lr {lg.get('lr', cfg.lr):.3e}  +{lg.get('lr_ups', 0):2d} -{lg.get('lr_downs', 0):2d}"
                         f"  kl {lg['approx_kl']:.5f}  ret {lg['avg_ep_rews']:8.2f}")
        final.setdefault(sched, []).append((sum(succ[-10:]) / len(succ[-10:]), max(succ)))
        print(lines[-1], name, flush=True)
        env.close()
        del tr
for sched, rows in final.items():
    lines.append(f"# {'adaptive' if sched else 'constant'}: success rate, mean of the last 10 iterations per seed: "
                 + ", ".join(f"{a:.4f}" for a, _ in rows) + "; best iteration per seed: " + ", ".join(f"{b:.4f}" for _, b in rows))
txt = "\n".join(lines) + "\n"
head = ""
if os.path.exists(args.out):
    old = open(args.out).read()
    k = old.find("# learning A/B")
    head = old if k < 0 else old[:k]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(head + txt)
print(txt[-800:])
