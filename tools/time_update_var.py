#!/usr/bin/env python3
"""Dev tool: what the learned exploration variance (navppo_*_update_epoch_var: the clipped epoch's launches as twins that read the
variance from the device state and carry one more per-lane sum, plus one small launch that steps log var) costs per epoch, per family
of fused kernels: the 2x64 heads on split-bf16 products and on the f32-input MFMA at 4096 x 512 samples, the 512-wide nets at
64 x 4096.  Two legs alternate in one process, `--rounds` (>= 5) rounds per family, timed with HIP events:
  clipped   E epochs of *_update_epoch_clipped
  var       E epochs of *_update_epoch_var (ent_coef 0.01)
Rule: the var median may exceed the clipped one by 1 % plus the clipped legs' own spread in this run.
usage: python tools/time_update_var.py [--rounds K] [--epochs E] [--out profiles/learned_var_epoch.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import nets, ppo

ap = argparse.ArgumentParser()
ap.add_argument("--n_heads", type=int, default=512 * 4096)
ap.add_argument("--n_wide", type=int, default=64 * 4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--max_norm", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "learned_var_epoch.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
if not torch.cuda.is_available():
    sys.exit("time_update_var: needs the GPU (there is no CPU timing of a HIP kernel)")

dev, E = torch.device("cuda"), args.epochs
lines = [f"# tools/time_update_var.py: {E}-epoch updates, {args.rounds} rounds of alternating legs, max_norm = {args.max_norm}, ent_coef = 0.01",
         f"# {torch.cuda.get_device_name(0)}; per-epoch times in us (update time / {E}), HIP events"]
ok = True
for policy, arith, n in (("mlp64x2", "bf16x3", args.n_heads), ("mlp64x2", "f32", args.n_heads), ("resmlp512", "bf16x3", args.n_wide)):
    g = torch.Generator().manual_seed(1)
    obs = torch.rand((n, 16), generator=g).to(dev)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(dev)
    logp = (-1.2 - 2.3 * torch.rand(n, generator=g)).to(dev)
    rtg = (torch.randn(n, generator=g) * 60 + 20).to(dev)
    adv = torch.randn(n, generator=g).to(dev)
    ups = {}
    for leg in ("clipped", "var"):
        torch.manual_seed(0)
        a, c = nets.make_policy(policy)
        a.to(dev), c.to(dev)
        cfg = ppo.PPOConfig(policy=policy, update_arith=arith, max_grad_norm=args.max_norm, learn_var=leg == "var",
                            ent_coef=0.01 if leg == "var" else 0.0)
        ups[leg] = ppo.PPOUpdater(a, c, cfg, None, dev)
        assert ups[leg].fused and ups[leg].bf16x3 == (policy == "mlp64x2" and arith == "bf16x3")
        if ups[leg].bf16x3:
            ups[leg].prepare(obs)
    st = torch.zeros(8, device=dev)
    cs = torch.zeros((E, 4), device=dev)

    def update(leg):
        up = ups[leg]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for ep in range(E):
            up._fused_epoch(obs, acts, logp, rtg, adv, 0.8, st, cs[ep])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / E

    legs = ("clipped", "var")
    for leg in legs:      # warm-up of every leg: code objects, workspaces
        update(leg)
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            t[leg].append(update(leg))
    med = {leg: statistics.median(v) for leg, v in t.items()}
    spread = max(t["clipped"]) - min(t["clipped"])
    allow = 0.01 * med["clipped"] + spread
    over = med["var"] - med["clipped"]
    ok = ok and over <= allow
    steps = ups["var"].var_state.tolist()
    name = "split-bf16" if arith == "bf16x3" and policy == "mlp64x2" else "f32 MFMA" if policy == "mlp64x2" else "512-wide nets"
    lines.append(f"{policy} ({name}), n = {n}:")
    for leg in legs:
        lines.append(f"  {leg:8s} median {med[leg]:10.1f}  min {min(t[leg]):10.1f}  max {max(t[leg]):10.1f}   legs: " + " ".join(f"{x:.1f}" for x in t[leg]))
    lines.append(f"  var - clipped = {over:+.1f} us ({100 * over / med['clipped']:+.2f} %); allowance 1 % + clipped spread = {allow:.1f} us: "
                 f"{'within' if over <= allow else 'EXCEEDED'}   (log var: {int(steps[5])} steps taken, {int(steps[6])} skipped, var {steps[1]:.4f})")
txt = "\n".join(lines) + "\n"
print(txt, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(txt)
sys.exit(0 if ok else 1)
