#!/usr/bin/env python3
"""Dev tool: what moving obstacles (navsim_set_movers) cost the persistent mlp64 rollout -- 4096 envs, stage_1, 512 steps per launch,
without a tape, with maps.orbit_movers at M = 32 (4 pillars x 8 sides) and M = 64 (4 x 16), and with a BANK of tapes
(navsim_set_mover_bank): maps.random_mover_bank(32, seed=0), one scenario per env, M = 32 as the first tape leg -- what differs from
that leg is the per-env row, which spreads the mover reads over the bank (a library without the entry point, e.g. a parent build
given as lib.so, runs without the bank leg).  The legs alternate in one
process (each leg a trainer of its own on the same device); per leg the median of 5 timed blocks of TM_REPS launches, and the
spread (max - min) of the no-tape leg's blocks, which is what a difference between legs has to exceed to mean anything.
--envs N: the shard size (default 4096, or TM_N).  --map NAME: the static map (default stage_1; "house": the 2048-segment tile-box map).
--shapes A,B,..: envs per workgroup forced on the rollout (navsim_set_shape; 0 = the rule), e.g. --shapes 16,64: every leg is then
timed once per shape ON THE SAME HANDLE, the shapes taking turns block by block -- the 16-env twin against the 64-env twin of a
handle with movers in one process (profiles/movers_big_rollout.txt).  --legs a,b: only the legs whose name contains one of these.
The tapes are authored geometry: parity unpinned (no reference geometry).
usage: python tools/time_movers.py [lib.so] [--envs N] [--map NAME] [--shapes 16,64] [--legs "no tape,M=32"] [> profiles/movers_rollout.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import _native, maps, ppo
from navbot_ppo_amd.env import VecEnv

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("lib", nargs="?", default=None, help="another build of libnavsim.so (e.g. the parent commit's)")
ap.add_argument("--envs", type=int, default=int(os.environ.get("TM_N", "4096")))
ap.add_argument("--map", default="stage_1")
ap.add_argument("--shapes", default="0", help="comma-separated envs per workgroup forced on the rollout; 0 = the rule")
ap.add_argument("--legs", default="", help="comma-separated substrings of the leg names to run (default: all)")
args = ap.parse_args()
if args.lib:
    _native.LIB_PATH = os.path.abspath(args.lib)
import ctypes
HAS_BANK = hasattr(ctypes.CDLL(_native.LIB_PATH), "navsim_set_mover_bank")
if not HAS_BANK:   # an older build: bind what it has
    _native.SYMBOLS = [s for s in _native.SYMBOLS if s[0] != "navsim_set_mover_bank"]
N, T, PERIOD = args.envs, int(os.environ.get("TM_T", "512")), int(os.environ.get("TM_PERIOD", "64"))
REPS, BLOCKS = int(os.environ.get("TM_REPS", "8")), 5
SHAPES = [int(x) for x in args.shapes.split(",")]
LEGS = [("no tape", None), ("orbit M=32", dict(tape=maps.orbit_movers(PERIOD, n=4, sides=8), phase="random")),
        ("orbit M=64", dict(tape=maps.orbit_movers(PERIOD, n=4, sides=16), phase="random"))]
if HAS_BANK:
    LEGS.append(("bank K=32", dict(name="random:32", seed=0)))
if args.legs:
    LEGS = [leg for leg in LEGS if any(w.strip() in leg[0] for w in args.legs.split(","))]

trainers = []
for name, movers in LEGS:
    env = VecEnv(N, map=args.map, max_episode_steps=500, seed=0, movers=movers)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", rollout_len=T, seed=0))
    assert tr.uses_persistent_rollout
    for shape in SHAPES:
        env.sim.set_shape(shape)
        for _ in range(2):
            tr.rollout()
    trainers.append((name, env, tr))
torch.cuda.synchronize()
ms = {(name, shape): [] for name, _ in LEGS for shape in SHAPES}
for _ in range(BLOCKS):
    for name, env, tr in trainers:   # the legs take turns, and within a leg the shapes
        for shape in SHAPES:
            env.sim.set_shape(shape)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                tr.rollout()
            e1.record()
            torch.cuda.synchronize()
            ms[(name, shape)].append(e0.elapsed_time(e1) / REPS)
print(f"persistent mlp64 rollout, {N} envs, {args.map}, {T} steps per launch, tape period {PERIOD}; {BLOCKS} blocks of {REPS} launches per leg, "
      f"legs alternating; library {os.path.relpath(_native.LIB_PATH)}; device {torch.cuda.get_device_name(0)}")
base = statistics.median(ms[(LEGS[0][0], SHAPES[0])])   # the first leg in its first shape (the no-tape leg unless --legs dropped it)
for name, env, tr in trainers:
    for shape in SHAPES:
        v = ms[(name, shape)]
        env.sim.set_shape(shape)
        inf = env.sim.info()
        done = int(tr.done_buf.sum())
        print(f"{name:<11s} forced {shape:<2d} median {statistics.median(v):7.3f} ms = {statistics.median(v) / T * 1e3:6.3f} us per step  (x{statistics.median(v) / base:5.3f})  "
              f"blocks {' '.join(f'{x:.3f}' for x in v)}  spread {max(v) - min(v):.3f} ms  rollout shape {inf['rollout_epb']} envs x {inf['rollout_waves']} waves "
              f"kind {inf['rollout_kind']} cast {inf['rollout_cast']}  collisions in the last rollout {done}")
    env.close()
print("tapes: authored geometry, parity unpinned (no reference geometry)")
