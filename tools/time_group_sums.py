#!/usr/bin/env python3
"""Dev tool: what PPOConfig.scenario_stats / scenario_priority cost.  Three parts, each appended to --out:
  kernel  navppo_group_sums at 512 x 4096, K = 32, with and without advantages, beside navppo_episode_sums on the same buffers (the
          yardstick): every leg a hipGraph of 32 calls, legs alternating in one process, median of --rounds, HIP events; microseconds and
          GB/s over the bytes the shapes say an entry point must read (flags 3, ep_length 4, ep_return 4, advantages 4 bytes per
          element; 4 bytes per env id; the workspace's round trip is the entry point's own business and is not counted)
  iter    whole iterations (4096 envs x 512 steps, 50 epochs, mlp64x2, movers random:32), a trainer with scenario_stats and one without,
          alternating in one process.  GATE: on <= off + 1 % + the off legs' own spread (exit status 1 otherwise)
  assign  one VecEnv.assign_scenarios call in ms (an existing entry point's cost: ids and phases checked on the host, the per-env spawn
          scans cast again), and the iteration with scenario_priority="failure" beside the two of `iter`; recorded, not gated
usage: python tools/time_group_sums.py [--parts kernel,iter,assign] [--rounds 5] [--out profiles/scenario_priority.txt]"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="kernel,iter,assign")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=512)
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--scenarios", type=int, default=32)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "scenario_priority.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
parts = args.parts.split(",")

sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from navbot_ppo_amd import ppo  # noqa: E402
from navbot_ppo_amd._native import _navppo, _ptr, lib  # noqa: E402
from navbot_ppo_amd.env import VecEnv  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_group_sums: needs the GPU (there is no CPU timing of a HIP kernel)")
dev = torch.device("cuda")
T, N, K = args.steps, args.envs, args.scenarios
status = 0


def emit(lines):
    txt = "\n".join(lines) + "\n"
    print(txt, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "a").write(txt)


def stat(v):
    return f"median {statistics.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f}"


def trainer(**cfg):
    env = VecEnv(N, map="stage_1", max_episode_steps=500, seed=0, movers=dict(name=f"random:{K}", seed=0))
    return ppo.PPOTrainer(env, ppo.PPOConfig(rollout_len=T, max_episode_steps=500, n_updates_per_iteration=args.epochs, policy="mlp64x2",
                                             seed=0, gae_lambda=0.95, **cfg))


emit([f"# tools/time_group_sums.py {time.strftime('%Y-%m-%d')}: {torch.cuda.get_device_name(0)}; parts {args.parts}"])

if "kernel" in parts:
    g = torch.Generator().manual_seed(0)
    ended = (torch.rand((T, N), generator=g) < 0.01).to(torch.uint8).to(dev)
    arrive = ((torch.rand((T, N), generator=g) < 0.5).to(torch.uint8).to(dev)) * ended
    done = ((torch.rand((T, N), generator=g) < 0.5).to(torch.uint8).to(dev)) * ended
    ep_len = (torch.randint(1, 500, (T, N), generator=g).to(torch.int32).to(dev)) * ended.int()
    ep_ret = (torch.rand((T, N), generator=g) * 200 - 100).to(dev)
    adv = torch.randn((T, N), generator=g).to(dev)
    group = torch.randint(0, K, (N,), generator=g).to(torch.int32).to(dev)
    out = torch.empty((K, 8), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib().navppo_group_sums_ws_bytes(T, N, K)), dtype=torch.uint8, device=dev)
    six, six_ws = torch.empty(6, dtype=torch.float64, device=dev), torch.empty(256 * 6, dtype=torch.float64, device=dev)
    legs = {"navppo_episode_sums": (lambda: _navppo("navppo_episode_sums", _ptr(ended), _ptr(arrive), _ptr(done), _ptr(ep_len), _ptr(ep_ret),
                                                     T * N, _ptr(six), _ptr(six_ws)), 11 * T * N),
            "navppo_group_sums": (lambda: ppo.group_sums(ended, arrive, done, ep_len, ep_ret, group, K, out=out, workspace=ws),
                                  11 * T * N + 4 * N),
            "navppo_group_sums, adv": (lambda: ppo.group_sums(ended, arrive, done, ep_len, ep_ret, group, K, adv=adv, out=out, workspace=ws),
                                       15 * T * N + 4 * N)}
    graphs = {}
    for leg, (fn, _) in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graphs[leg] = torch.cuda.CUDAGraph()   # 32 calls per replay: the python launch path is not what is measured
        with torch.cuda.graph(graphs[leg]):
            for _ in range(32):
                fn()
        graphs[leg].replay()
    torch.cuda.synchronize()
    ref = ppo.group_sums_reference(*(x.cpu().numpy() for x in (ended, arrive, done, ep_len, ep_ret, group)), K, adv=adv.cpu().numpy())
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [0, 1, 2, 3, 4, 7]], ref[:, [0, 1, 2, 3, 4, 7]]) and np.allclose(got[:, 5:7], ref[:, 5:7], rtol=1e-12, atol=0)
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
    lines = [f"(a) the entry points at {T} x {N}, K = {K} (workspace {ws.numel() / 2**20:.2f} MiB): hipGraph of 32 calls x 10 replays per figure, "
             f"{args.rounds} figures per leg, legs alternating; us per call (both launches of an entry point)"]
    for leg, (_, nbytes) in legs.items():
        us = statistics.median(t[leg])
        lines.append(f"  {leg:24s} {stat(t[leg])} us   {nbytes / 2**20:6.2f} MiB from the shapes -> {nbytes / us / 1e3:7.1f} GB/s")
    emit(lines)

if "iter" in parts or "assign" in parts:
    legs = {"scenario_stats off": trainer(), "scenario_stats on": trainer(scenario_stats=True)}
    if "assign" in parts:
        legs["scenario_priority failure"] = trainer(scenario_priority="failure")
    for tr in legs.values():
        tr.iteration()   # warm-up: code objects, workspaces
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, tr in legs.items():
            t[leg].append(tr.iteration()["iter_time"] * 1e3)
    lines = [f"(b) whole iterations, {N} envs x {T} steps, {args.epochs} epochs, mlp64x2, gae_lambda 0.95, movers random:{K}: {len(legs)} trainers "
             f"alternating in one process, {args.rounds} iterations each; ms per iteration (host wall clock around the iteration's one "
             "synchronisation; with scenario_priority the re-assignment lies behind it, outside this figure)"]
    for leg in legs:
        lines.append(f"  {leg:26s} {stat(t[leg])} ms   legs: " + " ".join(f"{x:.2f}" for x in t[leg]))
    off_legs = t["scenario_stats off"]
    off, on, spread = statistics.median(off_legs), statistics.median(t["scenario_stats on"]), max(off_legs) - min(off_legs)
    ok = on <= off * 1.01 + spread
    status |= 0 if ok else 1
    lines.append(f"  on - off = {on - off:+.3f} ms ({100 * (on - off) / off:+.2f} %); the off legs' own spread {spread:.3f} ms; "
                 f"GATE on <= off + 1 % + spread = {off * 1.01 + spread:.3f} ms: {'PASS' if ok else 'FAIL'}")
    if "assign" in parts:
        pr = statistics.median(t["scenario_priority failure"])
        lines.append(f"  scenario_priority - off = {pr - off:+.3f} ms ({100 * (pr - off) / off:+.2f} %) (recorded, not gated)")
        tr = legs["scenario_priority failure"]
        ms = []
        for _ in range(args.rounds):
            ids = tr.scenarios.assign(N)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.env.assign_scenarios(ids)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"(c) VecEnv.assign_scenarios, {N} envs over {K} scenarios, wall clock of the call and the stream behind it: {stat(ms)} ms "
                     "(recorded, not gated: navsim_set_mover_bank's checks on the host and the re-cast of the per-env spawn scans)")
        lines.append("    envs per scenario after the last iteration's scores: " + " ".join(str(c) for c in tr.scenarios.counts(N)))
    emit(lines)
    for tr in legs.values():
        tr.env.close()

sys.exit(status)
