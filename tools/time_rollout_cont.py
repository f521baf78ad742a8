#!/usr/bin/env python3
"""Dev tool: what continuing rollouts (PPOConfig.continue_rollouts) costs in the scan-history kernels.
  legs (default): in one process, alternating, medians of 5 timed blocks of THR_REPS launches at 4096 envs, stage_1, 512 steps:
     navsim_rollout_mlp64_hist | navsim_rollout_mlp64_hist_cont with null carries | ... with a carry out | ... with a carry in and out,
     and navsim_stack_rows | navsim_stack_rows_cont (null / in and out) on the rollout's [513, 4096, 16] buffer.  Recorded, not gated.
  --one: navsim_rollout_mlp64_hist alone, one line `hist_ms <median> <blocks...>` -- the leg of the gate against the parent commit:
     a driver runs this in fresh processes, this tree and the parent's alternating (NAVSIM_LIB names the library a process loads;
     the parent's tree runs its own copy of tools/time_rollout_hist.py's launch, which is this one).
usage: python tools/time_rollout_cont.py [--one] [>> profiles/continue_rollouts.txt]"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import ppo
from navbot_ppo_amd._native import _ptr, check, lib
from navbot_ppo_amd.env import VecEnv, stack_rows

N, T = int(os.environ.get("THR_N", "4096")), int(os.environ.get("THR_T", "512"))
REPS, BLOCKS = int(os.environ.get("THR_REPS", "8")), 5


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=0)
tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", rollout_len=T, seed=0, scan_history=True))
assert tr.uses_persistent_rollout


def launch(name, *carries):
    """reset + one persistent launch, as tools/time_rollout_hist.py times it"""
    env.sim.reset(tr.obs_buf[0])
    with torch.cuda.device(tr.device):
        check(getattr(lib(), name)(env.sim._h, _ptr(tr.updater.fp.flat), _ptr(tr.obs_buf), _ptr(tr.act_buf), _ptr(tr.logp_buf),
                                   _ptr(tr.rew_buf), _ptr(tr.done_buf), _ptr(tr.arrive_buf), _ptr(tr.ended_buf), _ptr(tr.epret_buf),
                                   _ptr(tr.eplen_buf), _ptr(tr.eppath_buf), _ptr(tr.var), tr._act_seed, _ptr(tr._step_base), T,
                                   *carries, C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def run(legs):
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(BLOCKS):
        for k, fn in legs.items():
            ms[k].append(timed(fn, REPS))
    return ms


if "--one" in sys.argv:
    v = run({"hist": lambda: launch("navsim_rollout_mlp64_hist")})["hist"]
    print("hist_ms", f"{statistics.median(v):.4f}", " ".join(f"{x:.4f}" for x in v))
    sys.exit(0)

print(f"history carries, {N} envs, stage_1, {T} steps per launch; {BLOCKS} blocks of {REPS} launches per leg, legs alternating; "
      f"device {torch.cuda.get_device_name(0)}")
ca, cb = (torch.zeros((N, 22), device=tr.device) for _ in range(2))
launch("navsim_rollout_mlp64_hist_cont", None, _ptr(ca))   # a real carry for the legs that read one
ms = run({"navsim_rollout_mlp64_hist": lambda: launch("navsim_rollout_mlp64_hist"),
          "navsim_rollout_mlp64_hist_cont null / null": lambda: launch("navsim_rollout_mlp64_hist_cont", None, None),
          "navsim_rollout_mlp64_hist_cont null / out": lambda: launch("navsim_rollout_mlp64_hist_cont", None, _ptr(cb)),
          "navsim_rollout_mlp64_hist_cont in / out": lambda: launch("navsim_rollout_mlp64_hist_cont", _ptr(ca), _ptr(cb))})
base = statistics.median(ms["navsim_rollout_mlp64_hist"])
for k, v in ms.items():
    print(f"{k:<44s} median {statistics.median(v):7.3f} ms = {statistics.median(v) / T * 1e3:6.3f} us per step (x{statistics.median(v) / base:5.3f})  "
          f"blocks {' '.join(f'{x:.3f}' for x in v)}  spread {max(v) - min(v):.3f} ms")
sr = run({"navsim_stack_rows": lambda: stack_rows(tr.obs_buf, tr.ended_buf, out=tr.hist_buf),
          "navsim_stack_rows_cont in / out": lambda: stack_rows(tr.obs_buf, tr.ended_buf, out=tr.hist_buf, carry_in=ca, carry_out=cb)})
gb = (T + 1) * N * (16 + 42) * tr.obs_buf.element_size() / 1e9
for k, v in sr.items():
    print(f"{k:<44s} [{T + 1}, {N}, 16] -> [.., 42]: median {statistics.median(v) * 1e3:7.1f} us = {gb / (statistics.median(v) * 1e-3):.0f} GB/s  "
          f"blocks {' '.join(f'{x * 1e3:.1f}' for x in v)}")
env.close()
