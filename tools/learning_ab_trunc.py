#!/usr/bin/env python3
"""Dev tool: the learning A/B of PPOConfig.bootstrap_truncated, recorded and not gated (three seeds on one map are a record, not a
claim).  mlp64x2, 4096 envs x 512 steps (stage_1, 500-step episodes), norm_reward=True, max_grad_norm=0.5, everything else the
defaults; legs off and on, for gae_lambda=None (the reference's estimator) and 0.95; seeds 0..2, `iterations` iterations each.  Per
iteration: training success rate, time-out rate (time-outs per finished episode), explained_variance of the critic before the update,
bootstrapped_frac, and every 10th iteration the deterministic evaluation's success rate (eval_every=10).
usage: python tools/learning_ab_trunc.py [iterations=60] [--seeds 3] [--out profiles/trunc_learning_ab.txt]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trunc_learning_ab.txt"))
args = ap.parse_args()
N, T = 4096, 512
lines = [f"# learning A/B (tools/learning_ab_trunc.py, {datetime.date.today().isoformat()}, {torch.cuda.get_device_name(0)}): mlp64x2, {N} envs x {T} steps, "
         f"{args.iterations} iterations, norm_reward, max_grad_norm 0.5, eval_every 10; bootstrap_truncated off against on, gae_lambda None and 0.95",
         "# per iteration: success rate | time-outs per finished episode | explained_variance | bootstrapped_frac | eval success (every 10th)"]
final = {}
for lam in (None, 0.95):
    for on in (False, True):
        for seed in range(args.seeds):
            env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed)
            cfg = ppo.PPOConfig(policy="mlp64x2", seed=seed, max_grad_norm=0.5, norm_reward=True, gae_lambda=lam, bootstrap_truncated=on,
                                eval_every=10)
            tr = ppo.PPOTrainer(env, cfg)
            name = f"gae_lambda {lam} bootstrap_truncated {'on' if on else 'off'} seed {seed}"
            lines.append(f"{name}:")
            succ, evals = [], []
            for it in range(1, args.iterations + 1):
                lg = tr.iteration()
                succ.append(lg["success_rate"])
                if "eval_success" in lg:
                    evals.append(lg["eval_success"])
                lines.append(f"  {it:3d}  succ {lg['success_rate']:.4f}  tmo {lg['timeouts'] / max(lg['episodes'], 1):.4f}  ev {lg['explained_variance']:7.4f}"
                             f"  boot {lg.get('bootstrapped_frac', 0.0):.5f}  ret {lg['avg_ep_rews']:8.2f}"
                             + (f"  eval {lg['eval_success']:.3f}" if "eval_success" in lg else ""))
            final.setdefault((lam, on), []).append((sum(succ[-10:]) / len(succ[-10:]), max(succ), evals[-1] if evals else float("nan")))
            print(lines[-1], name, flush=True)
            env.close()
            del tr
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write("\n".join(lines) + "\n")   # (a run that is cut short leaves the legs it finished)
for (lam, on), rows in final.items():
    lines.append(f"# gae_lambda {lam} {'on ' if on else 'off'}: success rate, mean of the last 10 iterations per seed: "
                 + ", ".join(f"{a:.4f}" for a, _, _ in rows) + "; best iteration per seed: " + ", ".join(f"{b:.4f}" for _, b, _ in rows)
                 + "; last evaluation per seed: " + ", ".join(f"{c:.3f}" for _, _, c in rows))
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines[-4:]))
