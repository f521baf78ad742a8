#!/usr/bin/env python3
"""Dev tool: what the adaptive learning rate (navppo_*_update_epoch_lr: the clipped epoch's launches, the step launch derives its rate
from approx_kl and the device state) costs per epoch, at the two headline sizes: 4096 x 512 samples for the 2x64 heads on split-bf16
products, 64 x 4096 samples for the 512-wide nets.  Two legs alternate in one process, `--rounds` (>= 5) rounds per family, timed with
HIP events:
  clipped   `--epochs` epochs of *_update_epoch_clipped
  lr        `--epochs` epochs of *_update_epoch_lr (adapt = 0 on the first, 1 on the others; the rule is free to move the rate)
The one rule, applied here: the lr median may exceed the clipped one by 1 % plus the clipped legs' own spread in this run -- the mode
adds no launch and a handful of scalar instructions to a launch that already exists, so anything more is a defect.
usage: python tools/time_update_lr.py [--rounds K] [--epochs E] [--out profiles/adaptive_lr_epoch.txt]   (the file's timing block is
replaced, what follows a line starting with "# learning A/B" is kept)"""
import argparse
import datetime
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import nets, ppo

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--max_norm", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adaptive_lr_epoch.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
if not torch.cuda.is_available():
    sys.exit("time_update_lr: needs the GPU (there is no CPU timing of a HIP kernel)")

dev, E = torch.device("cuda"), args.epochs
lines = [f"# tools/time_update_lr.py, {datetime.date.today().isoformat()}: {E}-epoch updates, {args.rounds} rounds of alternating legs, "
         f"max_norm = {args.max_norm}",
         f"# {torch.cuda.get_device_name(0)}; per-epoch times in us (update time / {E}), HIP events"]
ok = True
for policy, n in (("mlp64x2", 4096 * 512), ("resmlp512", 64 * 4096)):
    g = torch.Generator().manual_seed(1)
    obs = torch.rand((n, 16), generator=g).to(dev)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(dev)
    logp = (-1.2 - 2.3 * torch.rand(n, generator=g)).to(dev)
    rtg = (torch.randn(n, generator=g) * 60 + 20).to(dev)
    adv = torch.randn(n, generator=g).to(dev)
    ups = {}
    for kind, sched in (("clipped", None), ("lr", "adaptive")):
        torch.manual_seed(0)
        a, c = nets.make_policy(policy)
        a.to(dev), c.to(dev)
        ups[kind] = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, max_grad_norm=args.max_norm, lr_schedule=sched), None, dev)
        assert ups[kind].fused and ups[kind].bf16x3 == (policy == "mlp64x2")
        if ups[kind].bf16x3:
            ups[kind].prepare(obs)
    st = torch.zeros(8, device=dev)
    cs = torch.zeros((E, 4), device=dev)

    def update(leg):
        up = ups[leg]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for ep in range(E):
            up._fused_epoch(obs, acts, logp, rtg, adv, 0.8, st, cs[ep], adapt=ep > 0)   # (an update's first step does not adapt)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / E

    legs = ("clipped", "lr")
    for leg in legs:      # warm-up of every leg: code objects, workspaces
        update(leg)
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            t[leg].append(update(leg))
    med = {leg: statistics.median(v) for leg, v in t.items()}
    spread = max(t["clipped"]) - min(t["clipped"])
    allow = 0.01 * med["clipped"] + spread
    over = med["lr"] - med["clipped"]
    ok = ok and over <= allow
    lines.append(f"{policy} ({'split-bf16' if policy == 'mlp64x2' else '512-wide nets'}, n = {n}):")
    for leg in legs:
        lines.append(f"  {leg:8s} median {med[leg]:10.1f}  min {min(t[leg]):10.1f}  max {max(t[leg]):10.1f}   legs: " + " ".join(f"{x:.1f}" for x in t[leg]))
    lines.append(f"  lr - clipped = {over:+.1f} us ({100 * over / med['clipped']:+.2f} %); allowance 1 % + clipped spread = {allow:.1f} us: "
                 f"{'within' if over <= allow else 'EXCEEDED'}")
    lines.append(f"  rate state after the lr legs: {ups['lr'].lr_state.tolist()}")
txt = "\n".join(lines) + "\n"
print(txt, end="")
keep = ""
if os.path.exists(args.out):   # the learning A/B block (tools/learning_ab_lr.py) is appended to the same profile and survives a re-timing
    old = open(args.out).read()
    k = old.find("# learning A/B")
    keep = old[k:] if k >= 0 else ""
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(txt + keep)
sys.exit(0 if ok else 1)
