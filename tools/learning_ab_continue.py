#!/usr/bin/env python3
"""Dev tool: the learning A/B of PPOConfig.continue_rollouts, recorded and not gated (three seeds on one map are a record, not a
claim).  The configuration of tools/learning_ab_trunc.py -- mlp64x2, 4096 envs, stage_1, 500-step episodes, norm_reward=True,
max_grad_norm=0.5 -- with bootstrap_truncated=True on every leg (continuing needs a batch end that is not terminal), at EQUAL env-steps:
    rollout_len 512, every rollout from a reset | rollout_len 512 continuing | rollout_len 64 continuing (8 x the iterations)
Per leg and seed: the deterministic evaluation at the end (PPOTrainer.evaluate_now, 1000 episodes), the training success rate and the
explained_variance over the last tenth of the run, and the longest training episode seen.
usage: python tools/learning_ab_continue.py [iterations=60 (of 512 steps)] [--seeds 3] [--out profiles/continue_rollouts_learning.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "continue_rollouts_learning.txt"))
args = ap.parse_args()
N = 4096
LEGS = (("T 512 reset", 512, False), ("T 512 continue", 512, True), ("T 64 continue", 64, True))
lines = [f"# learning A/B (tools/learning_ab_continue.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, {N} envs, "
         f"{args.iterations} x 512 steps per env on every leg, norm_reward, max_grad_norm 0.5, bootstrap_truncated, gae_lambda None",
         "# per leg and seed: eval success / collision / time-out (deterministic, 1000 episodes, at the end) | training success rate and "
         "explained_variance, means of the last tenth of the iterations | longest training episode"]
for name, T, cont in LEGS:
    for seed in range(args.seeds):
        env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed)
        cfg = ppo.PPOConfig(policy="mlp64x2", seed=seed, rollout_len=T, max_grad_norm=0.5, norm_reward=True, bootstrap_truncated=True,
                            continue_rollouts=cont, eval_episodes=1000)
        tr = ppo.PPOTrainer(env, cfg)
        iters = args.iterations * 512 // T
        succ, ev, longest = [], [], 0
        for it in range(iters):
            lg = tr.iteration()
            succ.append(lg["success_rate"])
            ev.append(lg["explained_variance"])
            if it % max(iters // 10, 1) == 0 or it == iters - 1:
                longest = max(longest, int(tr.eplen_buf.max()))
        e = tr.evaluate_now()
        k = max(iters // 10, 1)
        lines.append(f"{name:<15s} seed {seed}: eval succ {e['eval_success']:.3f} coll {e['eval_collision']:.3f} tmo {e['eval_timeout']:.3f} | "
                     f"train succ {sum(succ[-k:]) / k:.4f}  ev {sum(ev[-k:]) / k:7.4f} | longest episode {longest} | {iters} iterations, "
                     f"{tr.env_steps} env-steps")
        print(lines[-1], flush=True)
        env.close()
        del tr
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
