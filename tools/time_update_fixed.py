#!/usr/bin/env python3
"""Dev tool: the fixed cost of one split-bf16 update epoch of the 16-64-64 heads (navppo_mlp64_bf16x3_update_epoch: the pass of both
nets in one launch, then the reduction with Adam) -- what an epoch costs besides its tiles: the launches, the prologue that splits the
weights into bf16 pieces (once per workgroup and net), the epilogues, the reduction and the gaps between the launches.  Times 20 epochs
on synthetic rows with HIP events at n = 32 * 1024 * k samples, k = 1, 2, 4 .. 64 (the pass runs 256 workgroups of 4 waves: k tiles per
wave and net), takes the median of 5 and fits  t(k) = intercept + slope * k  by least squares.  The intercept bounds what any change
to the per-launch work can win; the slope is the cost of a tile pair per wave.
--k 24,32,40,...: these tile counts instead (profiles/pass_pairing.txt: the marginal cost of a tile pair on either side of the batch size
that still fits the Infinity Cache), each row with its step from the row before.
usage: python tools/time_update_fixed.py [--label NAME] [--epochs E] [--reps R] [--k K1,K2,...] [--out profiles/x3s_fixed_cost.txt] [--append]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import nets, ppo

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="tree")
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--k", default="1,2,4,8,16,32,64", help="tiles per wave and net, ascending")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "x3s_fixed_cost.txt"))
ap.add_argument("--append", action="store_true", help="add this tree's block to --out instead of replacing the file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_update_fixed: needs the GPU (there is no CPU timing of a HIP kernel)")

dev = torch.device("cuda")
KS = tuple(int(k) for k in args.k.split(","))
assert len(KS) >= 2 and all(a < b for a, b in zip(KS, KS[1:])) and KS[0] >= 1, "--k: two or more ascending tile counts"
n_max = 32 * 1024 * KS[-1]
g = torch.Generator().manual_seed(1)
obs = torch.rand((n_max, 16), generator=g).to(dev)
acts = torch.stack([torch.rand(n_max, generator=g), torch.rand(n_max, generator=g) * 2 - 1], 1).to(dev)
logp = (-1.2 - 2.3 * torch.rand(n_max, generator=g)).to(dev)
rtg = (torch.randn(n_max, generator=g) * 60 + 20).to(dev)
adv = torch.randn(n_max, generator=g).to(dev)
torch.manual_seed(0)
a, c = nets.make_policy("mlp64x2")
a.to(dev), c.to(dev)
up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2"), None, dev)
assert up.fused and up.bf16x3
st = torch.zeros(8, device=dev)


def epochs_us(n):
    """per-epoch time of args.epochs epochs on the first n samples (contiguous prefixes of the same tensors)"""
    o, ac, lp, rt, ad = obs[:n], acts[:n], logp[:n], rtg[:n], adv[:n]
    up.prepare(o)
    up._fused_epoch(o, ac, lp, rt, ad, 0.8, st)   # warm-up at this size
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.epochs):
            up._fused_epoch(o, ac, lp, rt, ad, 0.8, st)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / args.epochs)
    return ts


lines = [f"# tools/time_update_fixed.py [{args.label}]: navppo_mlp64_bf16x3_update_epoch, {args.epochs} epochs between HIP events, median of "
         f"{args.reps}; {torch.cuda.get_device_name(0)}",
         "#   k = tiles per wave and net (n = 32 * 1024 * k samples); per-epoch times in us"]
med = []
for k in KS:
    ts = epochs_us(32 * 1024 * k)
    med.append(statistics.median(ts))
    step = f"  {(med[-1] - med[-2]) / (k - KS[len(med) - 2]):6.2f} us per tile pair from the row above" if len(med) > 1 else ""
    lines.append(f"  k = {k:2d}  n = {32 * 1024 * k:8d}  median {med[-1]:8.2f}  min {min(ts):8.2f}  max {max(ts):8.2f}{step}")
# least squares of t = a + b k over the points
mk, mt = sum(KS) / len(KS), sum(med) / len(med)
slope = sum((k - mk) * (t - mt) for k, t in zip(KS, med)) / sum((k - mk) ** 2 for k in KS)
icpt = mt - slope * mk
resid = max(abs(t - (icpt + slope * k)) for k, t in zip(KS, med))
lines.append(f"  fit [{args.label}]: intercept {icpt:.2f} us per epoch, slope {slope:.3f} us per tile pair and wave (largest residual {resid:.2f} us); "
             f"the intercept is {100 * icpt / med[-1]:.1f} % of the epoch at k = 64")
txt = "\n".join(lines) + "\n"
print(txt, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "a" if args.append else "w").write(txt)
