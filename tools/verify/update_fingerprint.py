#!/usr/bin/env python3
"""Dev tool: fingerprints of short training runs, to compare two checkouts bit for bit (a host-side refactor must not move one).
Per policy and config: 3 PPOTrainer.iteration()s of 64 envs x 32 steps on stage_1 with fixed seeds, then ONE line -- the SHA-256 over
the flat parameters and Adam's two moments, and the last iteration's statistics without the timing keys.  Run it in each checkout
(it imports the package it lies in) and compare the outputs with diff; a config whose line differs between two runs of the SAME
checkout does not reproduce itself and proves nothing either way.
usage: python tools/verify/update_fingerprint.py [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from navbot_ppo_amd import ppo  # noqa: E402
from navbot_ppo_amd.env import VecEnv  # noqa: E402

TIMING = ("rollout_time", "update_time", "iter_time", "steps_per_sec", "rollout_steps_per_sec")
CONFIGS = {"default": {},
           "minibatch": dict(minibatch_size=512, minibatch_shuffle="epoch"),
           "clip+kl": dict(max_grad_norm=0.5, target_kl=0.01),
           "adaptive_lr": dict(lr_schedule="adaptive"),
           "norm+trunc+gae": dict(norm_reward=True, bootstrap_truncated=True, gae_lambda=0.95)}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("update_fingerprint: needs the GPU (the fused update has no CPU build)")
lines = []
for policy in ("mlp64x2", "resmlp512"):
    for name, opts in CONFIGS.items():
        env = VecEnv(64, map="stage_1", max_episode_steps=12, seed=5, device="cuda:0")
        tr = ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=32, max_episode_steps=12, n_updates_per_iteration=4, policy=policy, seed=3, **opts))
        assert tr.updater.fused
        for _ in range(3):
            stats = tr.iteration()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (tr.updater.fp.flat, tr.updater._adam_m, tr.updater._adam_v):
            h.update(t.cpu().numpy().tobytes())
        lines.append(f"{policy} {name} {h.hexdigest()} " + json.dumps({k: stats[k] for k in sorted(stats) if k not in TIMING}))
        env.close()
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
