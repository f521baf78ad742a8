#!/usr/bin/env python3
"""Dev tool: what minibatch updates (PPOConfig.minibatch_size / minibatch_shuffle, navppo_shuffle_batch) cost, and that the full-batch
update costs what it did.  Four modes:
  legs   (default) one process, per policy -- the 2x64 heads on split-bf16 products at 4096 x 512 samples, the 512-wide nets at a batch
         that keeps a leg short -- whole updates alternating over the legs: the full batch, K in {8, 32} slices per epoch under each
         shuffle mode; then the shuffle kernel alone per row format (achieved bytes per second over the algorithmic 2 n (row bytes + 20)
         against the 8 TB/s peak) and shuffle + prepare.  Median of `--rounds` per leg, min .. max stated.  HIP events.
  kernel the last part of `legs` alone (an A/B build of the kernel: NAVSIM_LIB)
  full   the full-batch leg alone, of the package under --tree (this tree, or a checkout of another commit): one JSON line.
  gate   no GPU work of its own: starts `full` children of --tree and of --parent alternately, `--pairs` each, and applies the rule of
         tools/time_update_clip.py to the path that must not change: this tree's median may exceed the parent's by 1 % plus the parent
         legs' own spread in this run.
The text goes to --out (gate: appended to it).
usage: python tools/time_update_minibatch.py [--mode legs|kernel|full|gate] [--rounds R] [--epochs E] [--parent DIR] [--out profiles/minibatch_update.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="legs", choices=["legs", "kernel", "full", "gate"])
ap.add_argument("--tree", default=HERE, help="the checkout whose navbot_ppo_amd is timed")
ap.add_argument("--parent", default=None, help="gate: a built checkout of the parent commit")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--epochs", type=int, default=10)
ap.add_argument("--n_mlp64", type=int, default=512 * 4096)
ap.add_argument("--n_resmlp", type=int, default=64 * 4096)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "minibatch_update.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
SIZES = {"mlp64x2": args.n_mlp64, "resmlp512": args.n_resmlp}


def emit(lines, mode="w"):
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, mode).write(txt)


if args.mode == "gate":
    if not args.parent:
        ap.error("gate: --parent DIR")
    t = {"parent": {}, "this": {}}
    for _ in range(args.pairs):
        for tag, tree in (("parent", args.parent), ("this", args.tree)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "full", "--tree", tree, "--rounds", str(args.rounds),
                                "--epochs", str(args.epochs), "--n_mlp64", str(args.n_mlp64), "--n_resmlp", str(args.n_resmlp), "--out", os.devnull],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"time_update_minibatch: the {tag} leg failed ({r.returncode}):\n{r.stderr[-2000:]}")
            for policy, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                t[tag].setdefault(policy, []).extend(v)
    lines = ["", f"# the full-batch update against the parent commit: {args.pairs} processes per tree, alternating, {args.rounds} updates of {args.epochs} "
                 "epochs each; per-epoch times in us"]
    ok = True
    for policy in t["this"]:
        p, c = t["parent"][policy], t["this"][policy]
        mp, mc, spread = statistics.median(p), statistics.median(c), max(p) - min(p)
        allow = 0.01 * mp + spread
        ok &= mc - mp <= allow
        lines.append(f"{policy} (n = {SIZES[policy]}):")
        for tag, v, m in (("parent", p, mp), ("this", c, mc)):
            lines.append(f"  {tag:6s} median {m:9.1f}  min {min(v):9.1f}  max {max(v):9.1f}   legs: " + " ".join(f"{x:.1f}" for x in v))
        lines.append(f"  this - parent = {mc - mp:+.1f} us ({100 * (mc - mp) / mp:+.2f} %); allowance 1 % + the parent legs' spread = {allow:.1f} us: "
                     f"{'within' if mc - mp <= allow else 'EXCEEDED'}")
    emit(lines, "a")
    sys.exit(0 if ok else 1)

sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402
from navbot_ppo_amd import nets, ppo  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_update_minibatch: needs the GPU (there is no CPU timing of a HIP kernel)")
dev = torch.device("cuda")


def batch(n, D=16, dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    obs = torch.rand((n, D), generator=g).to(dtype).to(dev)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(dev)
    return obs, acts, (-1.2 - 2.3 * torch.rand(n, generator=g)).to(dev), (torch.randn(n, generator=g) * 60 + 20).to(dev)


def updater(policy, **cfg):
    torch.manual_seed(0)
    a, c = nets.make_policy(policy)
    a.to(dev), c.to(dev)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, n_updates_per_iteration=args.epochs, **cfg), None, dev)
    assert up.fused and (policy != "mlp64x2" or up.bf16x3)
    return up


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us


def stat(v):
    return f"median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}"


if args.mode == "full":
    out = {}
    for policy, n in SIZES.items():
        b, up = batch(n), updater(policy)
        run = lambda: up.update(*b, 0.8)
        run()
        out[policy] = [timed(run) / args.epochs for _ in range(args.rounds)]
    print(json.dumps(out))
    sys.exit(0)

lines = [f"# tools/time_update_minibatch.py: whole updates of {args.epochs} epochs (value pass, advantage normalisation and statistics included), legs "
         f"alternating in one process, {args.rounds} rounds; per-EPOCH times in us (update / {args.epochs}), HIP events",
         f"# {torch.cuda.get_device_name(0)}; K = slices per epoch = optimiser steps per epoch"]
for policy, n in (SIZES.items() if args.mode == "legs" else ()):
    b = batch(n)
    legs = {"full batch": updater(policy)}
    for K in (8, 32):
        for mode in ppo.MINIBATCH_SHUFFLES:
            legs[f"K={K:2d} {mode}"] = updater(policy, minibatch_size=n // K, minibatch_shuffle=mode)
    for up in legs.values():   # warm-up of every leg: code objects, workspaces, the permuted copy
        up.update(*b, 0.8)
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg, up in legs.items():
            t[leg].append(timed(lambda: up.update(*b, 0.8)) / args.epochs)
    base = statistics.median(t["full batch"])
    lines.append(f"{policy}, n = {n} samples:")
    for leg, v in t.items():
        lines.append(f"  {leg:12s} {stat(v)}   x{statistics.median(v) / base:6.3f}   legs: " + " ".join(f"{x:.1f}" for x in v))
    for K in (8, 32):
        d = statistics.median(t[f"K={K:2d} epoch"]) - statistics.median(t[f"K={K:2d} update"])
        lines.append(f"  K={K:2d}: a fresh permutation every epoch costs {d:+.1f} us per epoch over one per update")

# the kernel alone, per row format, and with the split of the permuted rows behind it (16- and 42-column float32 rows)
n = args.n_mlp64
lines.append(f"navppo_shuffle_batch alone, n = {n}: 20 launches per figure, {args.rounds} figures; algorithmic bytes 2 n (row bytes + 20); peak 8 TB/s")
for D, dtype in ((16, torch.float32), (16, torch.float16), (42, torch.float32), (42, torch.float16)):
    b = batch(n, D, dtype)
    adv = torch.randn(n, device=dev)
    torch.manual_seed(0)
    a, c = nets.make_policy("mlp64x2", D, 2)
    a.to(dev), c.to(dev)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2"), None, dev)
    full = (*b, adv)
    row = D * b[0].element_size()
    for what, bf16x3 in (("shuffle", False), ("shuffle + prepare", True)):
        up.bf16x3 = bf16x3
        up._shuffled(full, 1)
        v = [timed(lambda: up._shuffled(full, 7), 20) for _ in range(args.rounds)]
        bw = 2 * n * (row + 20) / (statistics.median(v) * 1e-6) / 1e12
        lines.append(f"  {row:3d}-byte rows  {what:17s} {stat(v)} us" + (f"   {bw:5.2f} TB/s = {100 * bw / 8:4.1f} % of peak" if not bf16x3 else ""))
emit(lines)
