#!/usr/bin/env python3
"""Dev tool: what PPOConfig.norm_reward costs and what it does to learning.  Three parts, each appended to --out:
  kernel  navppo_return_moments and navppo_reward_scale at 512 x 4096 against navsim_rtg_scan on the same buffers (the yardstick): every
          leg a hipGraph of 32 launches, legs alternating in one process, median of --rounds, HIP events; microseconds and achieved bytes per
          second over the algorithmic bytes (moments: 5 per element, scale: 8, return scan: 9)
  iter    whole iterations (4096 envs x 512 steps, 50 epochs, mlp64x2), a trainer with the option and one without, alternating in one
          process; the iteration time of each and the difference
  learn   --iters iterations of that configuration for the seeds --seeds, option off and on, both with max_grad_norm = 0.5: per iteration
          the success rate, the explained variance, the critic's loss and the share of optimiser steps whose critic gradient was clipped
usage: python tools/time_reward_norm.py [--parts kernel,iter,learn] [--rounds 5] [--iters 60] [--seeds 0,1,2] [--out profiles/reward_norm.txt]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="kernel,iter,learn")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--seeds", default="0,1,2")
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "reward_norm.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
parts = args.parts.split(",")

sys.path.insert(0, HERE)
import torch  # noqa: E402
from navbot_ppo_amd import ppo  # noqa: E402
from navbot_ppo_amd.env import VecEnv, rtg_scan  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_reward_norm: needs the GPU (there is no CPU timing of a HIP kernel)")
dev = torch.device("cuda")
T, N = args.steps, args.envs


def emit(lines):
    txt = "\n".join(lines) + "\n"
    print(txt, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write(txt)


def stat(v):
    return f"median {statistics.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f}"


def trainer(seed, **cfg):
    env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=seed)
    return ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=T, max_episode_steps=500, n_updates_per_iteration=args.epochs, policy="mlp64x2",
                                             seed=seed, **cfg))


emit([f"# tools/time_reward_norm.py {time.strftime('%Y-%m-%d')}: {torch.cuda.get_device_name(0)}; parts {args.parts}"])

if "kernel" in parts:
    g = torch.Generator().manual_seed(0)
    rew = (torch.rand((T, N), generator=g) * 50 - 25).to(dev)
    ended = (torch.rand((T, N), generator=g) < 0.01).to(torch.uint8).to(dev)
    out, scaled = torch.empty_like(rew), torch.empty_like(rew)
    rows = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    rms = torch.tensor([*ppo.RET_RMS_INIT, 0.0], dtype=torch.float64, device=dev)
    legs = {"navsim_rtg_scan": (lambda: rtg_scan(rew, ended, 0.99, out=out), 9),
            "navppo_return_moments": (lambda: ppo.return_moments(rew, ended, 0.99, out=rows[0]), 5),
            "navppo_reward_scale": (lambda: ppo.reward_scale(rms, rows, rew, out=scaled), 8)}
    graphs = {}
    for leg, (fn, _) in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graphs[leg] = torch.cuda.CUDAGraph()   # 32 launches per replay: the python launch path is not what is measured
        with torch.cuda.graph(graphs[leg]):
            for _ in range(32):
                fn()
        graphs[leg].replay()
    torch.cuda.synchronize()
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                graphs[leg].replay()
            e1.record()
            torch.cuda.synchronize()
            t[leg].append(e0.elapsed_time(e1) / 320 * 1e3)
    lines = [f"(a) the entry points at {T} x {N}: hipGraph of 32 calls x 10 replays per figure, {args.rounds} figures per leg, legs alternating; us per call"]
    for leg, (_, nbytes) in legs.items():
        us = statistics.median(t[leg])
        lines.append(f"  {leg:22s} {stat(t[leg])} us   {nbytes} B/element -> {T * N * nbytes / us / 1e6:5.2f} TB/s")
    emit(lines)
    kernel_us = statistics.median(t["navppo_return_moments"]) + statistics.median(t["navppo_reward_scale"])

if "iter" in parts:
    legs = {"norm_reward off": trainer(0), "norm_reward on": trainer(0, norm_reward=True)}
    for tr in legs.values():
        tr.iteration()   # warm-up: code objects, workspaces
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, tr in legs.items():
            t[leg].append(tr.iteration()["iter_time"] * 1e3)
    lines = [f"(b) whole iterations, {N} envs x {T} steps, {args.epochs} epochs, mlp64x2: two trainers alternating in one process, {args.rounds} iterations "
             "each; ms per iteration (host wall clock around the iteration's one synchronisation)"]
    for leg in legs:
        lines.append(f"  {leg:16s} {stat(t[leg])} ms   legs: " + " ".join(f"{x:.2f}" for x in t[leg]))
    off, on = (statistics.median(t[leg]) for leg in legs)
    lines.append(f"  on - off = {on - off:+.3f} ms ({100 * (on - off) / off:+.2f} %); the off legs' own spread {max(t['norm_reward off']) - min(t['norm_reward off']):.3f} ms")
    if "kernel" in parts:
        lines.append(f"  the two entry points of (a) together: {kernel_us:.1f} us = {100 * kernel_us * 1e-3 / off:.3f} % of one iteration")
    emit(lines)
    for tr in legs.values():
        tr.env.close()
    del legs

if "learn" in parts:
    seeds = [int(s) for s in args.seeds.split(",")]
    cols = ("success_rate", "explained_variance", "critic_loss", "grad_clip_frac_critic")
    res = {}
    for on in (False, True):
        for seed in seeds:
            tr = trainer(seed, norm_reward=on, max_grad_norm=0.5)
            seen = {}
            value = tr.updater.value   # (the critic's values before the update: what the update computes first)

            def remember(obs, value=value, seen=seen):
                seen["v0"] = value(obs)
                return seen["v0"]

            tr.updater.value = remember
            rows = []
            for _ in range(args.iters):
                lg = tr.iteration()
                if "explained_variance" not in lg:   # the option off: the same figure, from the same two tensors
                    tgt, v0 = tr.rtg_buf.reshape(-1).double(), seen["v0"].reshape(-1).double()
                    lg = dict(lg, explained_variance=float(1.0 - (tgt - v0).var(unbiased=False) / tgt.var(unbiased=False)))
                rows.append([lg[c] for c in cols])
            res[(on, seed)] = rows
            tr.env.close()
            print(f"[learn] norm_reward {'on' if on else 'off'}, seed {seed}: {args.iters} iterations done", flush=True)
    lines = [f"(c) learning, {N} envs x {T} steps, {args.epochs} epochs, mlp64x2, max_grad_norm = 0.5, seeds {seeds}: per iteration and leg, one value per seed",
             "    iter | leg | success_rate | explained_variance | critic_loss | grad_clip_frac_critic"]
    for it in range(args.iters):
        for on in (False, True):
            cells = [" ".join(f"{res[(on, s)][it][k]:.4g}" for s in seeds) for k in range(len(cols))]
            lines.append(f"    {it + 1:4d} | {'on ' if on else 'off'} | " + " | ".join(cells))
    for on in (False, True):
        clip = [res[(on, s)][it][3] for s in seeds for it in range(args.iters)]
        succ = [res[(on, s)][it][0] for s in seeds for it in range(args.iters - 10, args.iters)]
        lines.append(f"  norm_reward {'on ' if on else 'off'}: critic gradient clipped in {100 * statistics.mean(clip):.1f} % of the optimiser steps "
                     f"(mean over seeds and iterations); mean success rate of the last 10 iterations {statistics.mean(succ):.4f}")
    emit(lines)
