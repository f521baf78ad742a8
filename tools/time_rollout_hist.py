#!/usr/bin/env python3
"""Dev tool: what scan history (PPOConfig.scan_history) costs, recorded and not gated.
  1. the persistent rollout: navsim_rollout_mlp64 against navsim_rollout_mlp64_hist, 4096 envs, stage_1, 512 steps per launch, the two
     entry points alternating in one process, medians of 5 timed blocks of THR_REPS launches -- without movers and with
     maps.orbit_movers at M = 32 (4 pillars x 8 sides);
  2. navsim_stack_rows on the rollout's [513, 4096, 16] buffer against its byte count (rows read once + rows written once: the three
     reads of a row hit the caches);
  3. a whole iteration (rollout + return scan + 50-epoch update) with the option on and off.  The 42-column update runs the older
     compiler-scheduled split pass (about 1.1 ms per epoch against 0.68 for 16 columns, README, round-6 figures): most of the
     difference between the two iterations is that pass, not the history.
usage: python tools/time_rollout_hist.py [> profiles/scan_history.txt]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from navbot_ppo_amd import maps, ppo
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


def trainer(history, movers, **kw):
    env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=0, movers=movers)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(policy="mlp64x2", rollout_len=T, seed=0, scan_history=history, **kw))
    assert tr.uses_persistent_rollout
    return env, tr


print(f"scan history, {N} envs, stage_1, {T} steps per launch; {BLOCKS} blocks of {REPS} launches per leg, legs alternating; "
      f"device {torch.cuda.get_device_name(0)}")
# ---- 1. the rollout launch alone (reset + one persistent launch; the history leg without its navsim_stack_rows)
for mname, movers in (("no movers", None), ("orbit M=32", dict(tape=maps.orbit_movers(64, n=4, sides=8), phase="random"))):
    legs = [("navsim_rollout_mlp64", *trainer(False, movers)), ("navsim_rollout_mlp64_hist", *trainer(True, movers))]

    def launch(tr):
        tr.env.sim.reset(tr.obs_buf[0])
        tr._persistent_rollout()

    for _, _, tr in legs:
        for _ in range(2):
            launch(tr)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for _ in range(BLOCKS):
        for name, _, tr in legs:
            ms[name].append(timed(lambda: launch(tr), REPS))
    base = statistics.median(ms[legs[0][0]])
    for name, env, tr in legs:
        v = ms[name]
        print(f"{mname:<11s} {name:<26s} median {statistics.median(v):7.3f} ms = {statistics.median(v) / T * 1e3:6.3f} us per step  "
              f"(x{statistics.median(v) / base:5.3f})  blocks {' '.join(f'{x:.3f}' for x in v)}  spread {max(v) - min(v):.3f} ms")
        if name.endswith("_hist") and movers is None:   # ---- 2. navsim_stack_rows on this rollout's buffers
            sr = [timed(lambda: stack_rows(tr.obs_buf, tr.ended_buf, out=tr.hist_buf), REPS) for _ in range(BLOCKS)]
            es = tr.obs_buf.element_size()
            gb = (T + 1) * N * (16 + 42) * es / 1e9
            print(f"navsim_stack_rows [{T + 1}, {N}, 16] -> [.., 42] {tr.obs_buf.dtype}: median {statistics.median(sr) * 1e3:7.1f} us, "
                  f"{gb * 1e3:.1f} MB read once + written once = {gb / (statistics.median(sr) * 1e-3):.0f} GB/s  "
                  f"blocks {' '.join(f'{x * 1e3:.1f}' for x in sr)}")
        env.close()
# ---- 3. a whole iteration, option off / on
legs = [("scan_history off (16 columns)", *trainer(False, None)), ("scan_history on  (42 columns)", *trainer(True, None))]
for _, _, tr in legs:
    for _ in range(2):
        tr.iteration()
its = {name: [] for name, _, _ in legs}
for _ in range(BLOCKS):
    for name, _, tr in legs:
        lg = tr.iteration()
        its[name].append((lg["iter_time"] * 1e3, lg["rollout_time"] * 1e3, lg["update_time"] * 1e3))
for name, env, tr in legs:
    v = its[name]
    med = [statistics.median(x[k] for x in v) for k in range(3)]
    print(f"iteration, {name}: median {med[0]:7.2f} ms (rollout + scan {med[1]:6.2f}, update of {tr.cfg.n_updates_per_iteration} epochs {med[2]:6.2f} = "
          f"{med[2] / tr.cfg.n_updates_per_iteration:.3f} ms per epoch)  iterations {' '.join(f'{x[0]:.2f}' for x in v)}")
    env.close()
print("(the 42-column update runs the older compiler-scheduled split pass, about 1.1 ms per epoch against 0.68 for 16 columns in the "
      "README's round-6 figures: it is not touched here)")
