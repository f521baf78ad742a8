"""The precondition of tests/test_gpu_twins_wide.py's probe check of d/d(log var), on the CPU: for every shape of WIDE and both regimes
the probe batch is what its docstring says (every carrying probe's share at least a tenth of the largest, the masked ones exactly 0,
the closed form equal to float64 autograd), and PyTorch float32 autograd on the same batch errs by less than ONE TENTH of the bound the
GPU test holds the kernels to (a quarter of the smallest carrying probe's share).  If a case misses this, tighten the draw in
probe_batch (keep 1/2 q / var - 1 further from 0, or the floor higher) -- not the assertion."""
import pytest
import torch

import test_gpu_tails as tails
import test_gpu_twins_wide as tw


@pytest.mark.parametrize("regime", ["A", "B"])
@pytest.mark.parametrize("kind,D,f16,n", tw.SHAPES, ids=tw.wide_ids)
def test_float32_autograd_stays_below_a_tenth_of_the_probe_bound(monkeypatch, kind, D, f16, n, regime):
    monkeypatch.setattr(tails, "DEV", torch.device("cpu"))   # (the nets of the probe cases, built where this test runs)
    seed = n % 1000 + D
    actor, critic, _ = tw._nets(kind, D, seed)
    b = tw.probe_batch(actor, critic, kind, D, f16, n, regime, seed)
    g64, g32, bound = tw.probe_reference(actor, b, n)
    k, kc = b["pos"].numel(), int(b["carrying"].sum())
    print(f"{kind}-d{D}-{'f16' if f16 else 'f32'}-n{n} regime {regime}: {k} probes, {kc} carrying; float64 {g64:.9e}, bound {bound:.3e}, "
          f"float32 error / bound {abs(g32 - g64) / bound:.3e}")
    assert kc == (k if regime == "A" else (k + 1) // 2) and k >= 40
    assert int((b["adv"] != 0).sum()) == k and bool((b["adv"][b["pos"]] != 0).all())
    assert abs(g32 - g64) <= 0.1 * bound, (abs(g32 - g64), bound)
    # a probe dropped or counted twice, or a masked one left unmasked, misses the bound by a factor of 4 at the least
    t, rows = b["t"], b["rows"]
    assert float(t[b["carrying"]].abs().min()) / n >= 4 * bound * (1 - 1e-12)
    if regime == "B":
        unmasked = (rows["adv"].double() * rows["ratio"] * rows["h"])[~b["carrying"]].abs()
        assert float(unmasked.min()) / n >= 4 * bound * (1 - 1e-12)
        print(f"    the masked probes' terms, were they added: {float(unmasked.min()) / n / bound:.2f} .. {float(unmasked.max()) / n / bound:.2f} bounds")
