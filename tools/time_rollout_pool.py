#!/usr/bin/env python3
"""Dev tool: what the sector LiDAR (scan_pool) costs the persistent rollouts -- navsim_rollout_mlp64 at 4096 envs, stage_1, 512 steps
per launch, scan_pool k = 1 / 2 / 3 / 4, without movers and with maps.orbit_movers at M = 32, and the scan-history rollout
(navsim_rollout_mlp64_hist) at k = 1 / 4.  k = 1 is the kernel every handle without the option launches; k > 1 the pooled twin
(navsim_pool.hip: 16 envs on 8 waves, the mover and sensor-options form, stage B by entries).  The legs alternate in one process (each
leg a trainer of its own on the same device); per leg the median of 5 timed blocks of TP_REPS launches and the spread (max - min) of
its blocks, which is what a difference between legs has to exceed to mean anything.
usage: python tools/time_rollout_pool.py [--envs N] [--map NAME] [>> profiles/scan_pool.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd.env import VecEnv

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--envs", type=int, default=int(os.environ.get("TP_N", "4096")))
ap.add_argument("--map", default="stage_1")
args = ap.parse_args()
N, T, PERIOD = args.envs, int(os.environ.get("TP_T", "512")), 64
REPS, BLOCKS = int(os.environ.get("TP_REPS", "8")), 5
TAPE = dict(tape=maps.orbit_movers(PERIOD, n=4, sides=8), phase="random")
LEGS = [(f"{world:<10s} {'history' if hist else 'rows16 '} k={k}", movers, hist, k)
        for world, movers in (("no movers", None), ("orbit M=32", TAPE)) for hist, ks in ((False, (1, 2, 3, 4)), (True, (1, 4))) for k in ks]

trainers = []
for name, movers, hist, k in LEGS:
    env = VecEnv(N, map=args.map, max_episode_steps=500, seed=0, movers=movers, scan_pool=k)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", rollout_len=T, seed=0, scan_history=hist))
    assert tr.uses_persistent_rollout and env.sim.info()["scan_pool"] == k
    for _ in range(2):
        tr.rollout()
    trainers.append((name, env, tr))
torch.cuda.synchronize()
ms = {name: [] for name, *_ in LEGS}
for _ in range(BLOCKS):
    for name, env, tr in trainers:   # the legs take turns
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            tr.rollout()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / REPS)
print(f"persistent mlp64 rollouts under scan_pool, {N} envs, {args.map}, {T} steps per launch, tape period {PERIOD}; {BLOCKS} blocks of "
      f"{REPS} launches per leg, legs alternating; device {torch.cuda.get_device_name(0)}")
for name, env, tr in trainers:
    v = ms[name]
    base = statistics.median(ms[name[:-1] + "1"])   # the k = 1 leg of the same world and policy
    inf = env.sim.info()
    print(f"  {name}: {statistics.median(v):7.3f} ms per rollout = {1e3 * statistics.median(v) / T:6.3f} us per step "
          f"({1e3 * (statistics.median(v) - base) / T:+6.3f} us over k=1; blocks {min(v):.3f}-{max(v):.3f}, spread {max(v) - min(v):.3f} ms); "
          f"{inf['rollout_epb']} envs on {inf['rollout_waves']} waves, cast {inf['rollout_cast']}; collisions in the last rollout "
          f"{int(tr.done_buf.sum())}")
    env.close()
