"""Dev tool: navsim_rtg_scan timing (hipGraph of 32 launches, HIP events) for the T-split kernel and the serial (bit-exact) one,
plus the share of stores that differ from the oracle (contract: <= 1 float32 ulp), and navsim_gae_scan beside navsim_gae_scan_trunc."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, numpy as np
from navbot_ppo_amd.env import rtg_scan
from oracle import navsim_oracle as O
for T, N, p in ((512, 4096, .01), (512, 4096, .001), (512, 4096, 0.), (512, 4097, .01), (100, 37, .01), (1300, 640, .002)):
    rew = torch.randn((T, N), device="cuda") * 20; ended = (torch.rand((T, N), device="cuda") < p).to(torch.uint8)
    out = rtg_scan(rew, ended, 0.99).cpu().numpy()
    ref = O.compute_rtgs_tn(rew.cpu().numpy(), ended.cpu().numpy(), 0.99)
    d = np.abs(out.view(np.int32).astype(np.int64) - ref.view(np.int32))
    print(f"T={T} N={N} p_end={p}: max ulp {d.max()}, differing stores {(d != 0).sum()} of {d.size}")
    assert d.max() <= 1
T, N = 512, 4096
rew = torch.randn((T, N), device="cuda"); ended = (torch.rand((T, N), device="cuda") < 0.01).to(torch.uint8); out = torch.empty_like(rew)
for mode in ("0", "1"):
    ex = mode == "1"
    for _ in range(10): rtg_scan(rew, ended, 0.99, out=out, exact=ex)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()   # 32 launches per replay: the python launch path is not what is measured
    with torch.cuda.graph(g):
        for _ in range(32): rtg_scan(rew, ended, 0.99, out=out, exact=ex)
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): g.replay()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 320 * 1e3
    print(f"rtg_scan {T}x{N} {'serial (exact)' if mode == '1' else 'T-split'}: {us:.2f} us -> {T*N*9/us/1e3:.1f} GB/s")

# navsim_gae_scan beside navsim_gae_scan_trunc on the same buffers (1 % episode ends, a third of them time-outs), the two legs alternating
# in one process, medians of 5: the truncation-aware form reads two more byte streams (19 bytes per element instead of 17)
from navbot_ppo_amd.env import gae_scan, gae_scan_trunc
kind = torch.randint(0, 3, (T, N), device="cuda")
done, arrive = ended * (kind == 0).to(torch.uint8), ended * (kind == 1).to(torch.uint8)
val = torch.randn((T, N), device="cuda"); lastv = torch.randn(N, device="cuda")
legs = {"gae_scan": (lambda ex: gae_scan(rew, ended, val, 0.99, 0.95, last_value=lastv, exact=ex), 17),
        "gae_scan_trunc": (lambda ex: gae_scan_trunc(rew, ended, done, arrive, val, 0.99, 0.95, last_value=lastv, exact=ex), 19)}
for ex in (False, True):
    graphs, times = {}, {k: [] for k in legs}
    for name, (fn, _) in legs.items():
        for _ in range(10): fn(ex)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(32): fn(ex)
        graphs[name].replay(); torch.cuda.synchronize()
    for rep in range(5):
        for name in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10): graphs[name].replay()
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 320 * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name, (_, nbytes) in legs.items():
        print(f"{name} {T}x{N} {'serial (exact)' if ex else 'T-split'}: median of 5 {med[name]:.2f} us (min {min(times[name]):.2f} max {max(times[name]):.2f})"
              f" -> {T*N*nbytes/med[name]/1e3:.1f} GB/s")
    print(f"gae_scan_trunc / gae_scan {'serial (exact)' if ex else 'T-split'}: {med['gae_scan_trunc'] / med['gae_scan']:.3f} (19 / 17 bytes = 1.118)")
