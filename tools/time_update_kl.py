#!/usr/bin/env python3
"""Dev tool: what the early stop at a KL limit (navppo_*_update_epoch_kl: the clipped epoch's launches as gated twins, the decision in
the step launch) costs and saves, at the headline batch: 4096 x 512 samples, per family of fused kernels -- the 2x64 heads on
split-bf16 products and on the f32-input MFMA (16 columns), and the 512-wide nets.  Four legs alternate in one process, `--rounds`
(>= 5) rounds per family, timed with HIP events:
  clipped   50 epochs of *_update_epoch_clipped
  kl        50 epochs of *_update_epoch_kl that never trip (kl_limit = +inf)
  stopped   50 epochs of *_update_epoch_kl on a state whose stopped flag is set: every kernel returns at its entry
  stop10    a 50-epoch update that stops after 10 epochs: 10 executed epochs, the flag set on the stream, 40 stopped ones
Rules: (a) the kl median may exceed the clipped one by 1 % plus the clipped legs' own spread in this run; (b) a stopped epoch is below
an executed one for every family (all of them ship gated passes) -- otherwise the gate is not working.
usage: python tools/time_update_kl.py [--n N] [--rounds K] [--epochs E] [--out profiles/kl_stop_epoch.txt]"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from navbot_ppo_amd import nets, ppo

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512 * 4096)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--max_norm", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kl_stop_epoch.txt"))
args = ap.parse_args()
if args.rounds < 5:
    ap.error("--rounds: at least 5")
if not torch.cuda.is_available():
    sys.exit("time_update_kl: needs the GPU (there is no CPU timing of a HIP kernel)")

n, dev, E = args.n, torch.device("cuda"), args.epochs
K10 = min(10, E)
g = torch.Generator().manual_seed(1)
obs = torch.rand((n, 16), generator=g).to(dev)
acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1).to(dev)
logp = (-1.2 - 2.3 * torch.rand(n, generator=g)).to(dev)
rtg = (torch.randn(n, generator=g) * 60 + 20).to(dev)
adv = torch.randn(n, generator=g).to(dev)
lines = [f"# tools/time_update_kl.py: n = {n} samples, {E}-epoch updates, {args.rounds} rounds of alternating legs, max_norm = {args.max_norm}",
         f"# {torch.cuda.get_device_name(0)}; per-epoch times in us (update time / {E}), HIP events; stop10: the whole update in us"]
ok = True
for policy, arith in (("mlp64x2", "bf16x3"), ("mlp64x2", "f32"), ("resmlp512", "bf16x3")):
    ups = {}
    for kind, tkl in (("clipped", None), ("kl", 1.0)):
        torch.manual_seed(0)
        a, c = nets.make_policy(policy)
        a.to(dev), c.to(dev)
        ups[kind] = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy=policy, update_arith=arith, max_grad_norm=args.max_norm, target_kl=tkl), None, dev)
        assert ups[kind].fused and ups[kind].bf16x3 == (policy == "mlp64x2" and arith == "bf16x3")
        if ups[kind].bf16x3:
            ups[kind].prepare(obs)
    ups["kl"].kl_limit = math.inf   # never trips
    st = torch.zeros(8, device=dev)
    cs = torch.zeros((E, 4), device=dev)
    flag = torch.ones((), device=dev)

    def update(leg):
        up = ups["clipped" if leg == "clipped" else "kl"]
        if leg != "clipped":
            up.kl_state = torch.zeros(4, device=dev)
            if leg == "stopped":
                up.kl_state[0] = 1.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for ep in range(E):
            if leg == "stop10" and ep == K10:
                up.kl_state[0:1].copy_(flag)   # on the stream, no host round trip: what the step launch of a tripping epoch does
            up._fused_epoch(obs, acts, logp, rtg, adv, 0.8, st, cs[ep])
        e1.record()
        torch.cuda.synchronize()
        if leg == "stop10":
            assert up.kl_state.tolist()[:2] == [1.0, float(K10)]
        return e0.elapsed_time(e1) * 1e3 / (1 if leg == "stop10" else E)

    legs = ("clipped", "kl", "stopped", "stop10")
    for leg in legs:      # warm-up of every leg: code objects, workspaces
        update(leg)
    t = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            t[leg].append(update(leg))
    med = {leg: statistics.median(v) for leg, v in t.items()}
    spread = max(t["clipped"]) - min(t["clipped"])
    allow = 0.01 * med["clipped"] + spread
    over = med["kl"] - med["clipped"]
    a_ok, b_ok = over <= allow, med["stopped"] < med["kl"]
    ok = ok and a_ok and b_ok
    lines.append(f"{policy} ({'split-bf16' if arith == 'bf16x3' and policy == 'mlp64x2' else 'f32 MFMA' if policy == 'mlp64x2' else '512-wide nets'}):")
    for leg in legs:
        lines.append(f"  {leg:8s} median {med[leg]:10.1f}  min {min(t[leg]):10.1f}  max {max(t[leg]):10.1f}   legs: " + " ".join(f"{x:.1f}" for x in t[leg]))
    lines.append(f"  (a) kl - clipped = {over:+.1f} us ({100 * over / med['clipped']:+.2f} %); allowance 1 % + clipped spread = {allow:.1f} us: "
                 f"{'within' if a_ok else 'EXCEEDED'}")
    lines.append(f"  (b) stopped epoch {med['stopped']:.1f} us = {med['stopped'] / med['kl']:.4f} of an executed one ({med['kl']:.1f} us): "
                 f"{'below' if b_ok else 'NOT BELOW'}")
    lines.append(f"      {E}-epoch update stopped after {K10} epochs: {med['stop10'] / 1e3:.2f} ms against {med['kl'] * E / 1e3:.2f} ms for all {E} "
                 f"({med['stop10'] / (med['kl'] * E):.3f})")
txt = "\n".join(lines) + "\n"
print(txt, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(txt)
sys.exit(0 if ok else 1)
