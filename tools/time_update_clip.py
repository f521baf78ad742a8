#!/usr/bin/env python3
"""Dev tool: what the clipped update epoch (navppo_*_update_epoch_clipped: one more small launch that sums the squared-norm slots,
clips and runs Adam) costs over the existing epoch (Adam inside the reduction), at the headline batch: 4096 x 512 samples, the 2x64
heads on split-bf16 products at 16 columns, and the 512-wide nets.  50-epoch updates through either entry point alternate in one
process, `--pairs` (>= 5) pairs per policy, timed with HIP events; per-epoch medians and each leg's min-max go to the output file.
The rule it applies: the clipped median may exceed the unclipped one by 1 % plus the unclipped legs' own spread in this run.
usage: python tools/time_update_clip.py [--n N] [--pairs K] [--epochs E] [--out profiles/grad_clip_epoch.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import nets, ppo

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512 * 4096)
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--max_norm", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_clip_epoch.txt"))
args = ap.parse_args()
if args.pairs < 5:
    ap.error("--pairs: at least 5")
if not torch.cuda.is_available():
    sys.exit("time_update_clip: needs the GPU (there is no CPU timing of a HIP kernel)")

n, dev = args.n, torch.device("cuda")
g = torch.Generator().manual_seed(1)
obs = torch.rand((n, 16), generator=g).to(dev)
acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(dev)
logp = (-1.2 - 2.3 * torch.rand(n, generator=g)).to(dev)
rtg = (torch.randn(n, generator=g) * 60 + 20).to(dev)
adv = torch.randn(n, generator=g).to(dev)
lines = [f"# tools/time_update_clip.py: n = {n} samples, {args.epochs}-epoch updates, {args.pairs} alternating pairs, max_norm = {args.max_norm}",
         f"# {torch.cuda.get_device_name(0)}; per-epoch times in us (update time / {args.epochs}), HIP events"]
for policy in ("mlp64x2", "resmlp512"):
    ups = {}
    for leg, mgn in (("unclipped", None), ("clipped", args.max_norm)):
        torch.manual_seed(0)
        a, c = nets.make_policy(policy)
        a.to(dev), c.to(dev)
        ups[leg] = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, max_grad_norm=mgn), None, dev)
        assert ups[leg].fused and (policy != "mlp64x2" or ups[leg].bf16x3)
        if ups[leg].bf16x3:
            ups[leg].prepare(obs)
    st = torch.zeros(8, device=dev)
    cs = torch.zeros((args.epochs, 4), device=dev)

    def update(leg):
        up = ups[leg]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for ep in range(args.epochs):
            up._fused_epoch(obs, acts, logp, rtg, adv, 0.8, st, cs[ep] if leg == "clipped" else None)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.epochs

    for leg in ups:      # warm-up of both legs: code objects, workspaces
        update(leg)
    t = {leg: [] for leg in ups}
    for _ in range(args.pairs):
        for leg in ("unclipped", "clipped"):
            t[leg].append(update(leg))
    med = {leg: statistics.median(v) for leg, v in t.items()}
    spread = max(t["unclipped"]) - min(t["unclipped"])
    allow = 0.01 * med["unclipped"] + spread
    over = med["clipped"] - med["unclipped"]
    frac = float((cs[:, 2:] < 1).float().mean())
    lines.append(f"{policy}:")
    for leg in ("unclipped", "clipped"):
        lines.append(f"  {leg:9s} median {med[leg]:9.1f}  min {min(t[leg]):9.1f}  max {max(t[leg]):9.1f}   legs: " + " ".join(f"{x:.1f}" for x in t[leg]))
    lines.append(f"  clipped - unclipped = {over:+.1f} us ({100 * over / med['unclipped']:+.2f} %); allowance 1 % + unclipped spread = {allow:.1f} us: "
                 f"{'within' if over <= allow else 'EXCEEDED'}   (share of clipped (net, epoch) pairs in the last update: {frac:.2f})")
txt = "\n".join(lines) + "\n"
print(txt, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(txt)
