#!/usr/bin/env python3
"""Dev tool: what moving obstacles (navsim_set_movers) cost the persistent mlp64 rollout -- 4096 envs, stage_1, 512 steps per launch,
without a tape, with maps.orbit_movers at M = 32 (4 pillars x 8 sides) and M = 64 (4 x 16), and with a BANK of tapes
(navsim_set_mover_bank): maps.random_mover_bank(32, seed=0), one scenario per env, M = 32 as the first tape leg -- what differs from
that leg is the per-env row, which spreads the mover reads over the bank (a library without the entry point, e.g. a parent build
given as lib.so, runs without the bank leg).  The legs alternate in one
process (each leg a trainer of its own on the same device); per leg the median of 5 timed blocks of TM_REPS launches, and the
spread (max - min) of the no-tape leg's blocks, which is what a difference between legs has to exceed to mean anything.
The tapes are authored geometry: parity unpinned (no reference geometry).
usage: python tools/time_movers.py [lib.so] [> profiles/movers_rollout.txt]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import _native, maps, ppo
from navbot_ppo_amd.env import VecEnv

_libs = [a for a in sys.argv[1:] if a.endswith(".so")]
if _libs:
    _native.LIB_PATH = os.path.abspath(_libs[0])
import ctypes
HAS_BANK = hasattr(ctypes.CDLL(_native.LIB_PATH), "navsim_set_mover_bank")
if not HAS_BANK:   # an older build: bind what it has
    _native.SYMBOLS = [s for s in _native.SYMBOLS if s[0] != "navsim_set_mover_bank"]
N, T, PERIOD = int(os.environ.get("TM_N", "4096")), int(os.environ.get("TM_T", "512")), int(os.environ.get("TM_PERIOD", "64"))
REPS, BLOCKS = int(os.environ.get("TM_REPS", "8")), 5
LEGS = [("no tape", None), ("orbit M=32", dict(tape=maps.orbit_movers(PERIOD, n=4, sides=8), phase="random")),
        ("orbit M=64", dict(tape=maps.orbit_movers(PERIOD, n=4, sides=16), phase="random"))]
if HAS_BANK:
    LEGS.append(("bank K=32", dict(name="random:32", seed=0)))

trainers = []
for name, movers in LEGS:
    env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=0, movers=movers)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", rollout_len=T, seed=0))
    assert tr.uses_persistent_rollout
    for _ in range(2):
        tr.rollout()
    trainers.append((name, env, tr))
torch.cuda.synchronize()
ms = {name: [] for name, _ in LEGS}
for _ in range(BLOCKS):
    for name, env, tr in trainers:   # the legs take turns
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            tr.rollout()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / REPS)
print(f"persistent mlp64 rollout, {N} envs, stage_1, {T} steps per launch, tape period {PERIOD}; {BLOCKS} blocks of {REPS} launches per leg, "
      f"legs alternating; device {torch.cuda.get_device_name(0)}")
base = statistics.median(ms["no tape"])
for name, env, tr in trainers:
    v = ms[name]
    inf = env.sim.info()
    done = int(tr.done_buf.sum())
    print(f"{name:<11s} median {statistics.median(v):7.3f} ms = {statistics.median(v) / T * 1e3:6.3f} us per step  (x{statistics.median(v) / base:5.3f})  "
          f"blocks {' '.join(f'{x:.3f}' for x in v)}  spread {max(v) - min(v):.3f} ms  rollout shape {inf['rollout_epb']} envs x {inf['rollout_waves']} waves "
          f"kind {inf['rollout_kind']}  collisions in the last rollout {done}")
    env.close()
print("tapes: authored geometry, parity unpinned (no reference geometry)")
