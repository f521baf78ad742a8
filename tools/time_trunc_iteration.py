#!/usr/bin/env python3
"""Dev tool: what PPOConfig.bootstrap_truncated costs per iteration, recorded and not gated.  Whole iterations (4096 envs x 512 steps, 50
epochs, mlp64x2), trainers with the option off and on, for gae_lambda None and 0.95, alternating in one process, medians of --rounds.
With the option the rollout computes V of all T + 1 stored rows (gae_lambda None: the update no longer computes V0 itself, so the value
pass grows by N rows, it is not added) and the scan reads two more byte streams.  Appended to --out.
usage: python tools/time_trunc_iteration.py [--rounds 5] [--out profiles/trunc_scan.txt]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "trunc_scan.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")

sys.path.insert(0, HERE)
import torch  # noqa: E402
from navbot_ppo_amd import ppo  # noqa: E402
from navbot_ppo_amd.env import VecEnv  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_trunc_iteration: needs the GPU")
T, N = args.steps, args.envs


def trainer(**cfg):
    env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=0)
    return ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=T, max_episode_steps=500, policy="mlp64x2", seed=0, **cfg))


legs = {f"gae_lambda {lam} bootstrap_truncated {'on ' if on else 'off'}": trainer(gae_lambda=lam, bootstrap_truncated=on)
        for lam in (None, 0.95) for on in (False, True)}
for tr in legs.values():
    tr.iteration()   # warm-up: code objects, workspaces
t = {leg: [] for leg in legs}
for _ in range(args.rounds):
    for leg, tr in legs.items():
        t[leg].append(tr.iteration()["iter_time"] * 1e3)
lines = [f"# tools/time_trunc_iteration.py {time.strftime('%Y-%m-%d')}: {torch.cuda.get_device_name(0)}",
         f"whole iterations, {N} envs x {T} steps, 50 epochs, mlp64x2: four trainers alternating in one process, {args.rounds} iterations each; ms per "
         "iteration (host wall clock around the iteration's one synchronisation)"]
for leg, v in t.items():
    lines.append(f"  {leg}  median {statistics.median(v):8.2f}  min {min(v):8.2f}  max {max(v):8.2f} ms   legs: " + " ".join(f"{x:.2f}" for x in v))
names = list(legs)
for off, on in ((names[0], names[1]), (names[2], names[3])):
    a, b = statistics.median(t[off]), statistics.median(t[on])
    lines.append(f"  {on.strip()} - off = {b - a:+.3f} ms ({100 * (b - a) / a:+.2f} %); the off leg's own spread {max(t[off]) - min(t[off]):.3f} ms")
txt = "\n".join(lines) + "\n"
print(txt, end="", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "a").write(txt)
for tr in legs.values():
    tr.env.close()
