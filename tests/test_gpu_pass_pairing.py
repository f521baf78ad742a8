"""GPU tests of the workgroup pairing of the split-bf16 update pass (csrc/ppo_mlp64_x3s.h: mlp64_pass_both_x3s, X3S_PAIR).  A both-nets
launch whose grid is a multiple of 16 workgroups pairs workgroup b with b ^ 8: one runs the actor, the other the critic over the SAME
tiles, then they swap, so that a tile is fetched once per epoch.  Which workgroup computes a partial row must not change a bit of it:
  * the gradient and the statistics of one navppo_mlp64_bf16x3_loss_grad launch (both nets, paired where the grid allows) equal those of
    navppo_mlp64_bf16x3_loss_grad_net(0) followed by (1) (single-net launches: never paired, the same tiles per row) bit for bit;
  * one navppo_mlp64_bf16x3_update_epoch leaves the parameters and Adam's moments bit-identical to a library built with -DX3S_PAIR=0
    (tools/build_mlp64_variant.py).
Grid: min(ceil(tiles / 8), 256) workgroups of 4 waves (csrc/ppo_mlp64.hip: plan_pass), tiles of 32 samples."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from navbot_ppo_amd import _native, nets, ppo

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((n, 16), generator=g)
    acts = torch.stack([torch.rand(n, generator=g), torch.rand(n, generator=g) * 2 - 1], 1)
    logp = -1.2 - 2.3 * torch.rand(n, generator=g)
    rtg = torch.randn(n, generator=g) * 60 + 20
    adv = torch.randn(n, generator=g)
    return [t.to(dev).contiguous() for t in (obs, acts, logp, rtg, adv)]


def _updater(dev, seed=3):
    torch.manual_seed(seed)
    a, c = nets.make_policy("mlp64x2", 16)
    a.to(dev), c.to(dev)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2"), None, dev)
    assert up.fused_mlp64 and up.bf16x3
    return up


# 4096: 16 workgroups, one pair group; 4091: a ragged last tile inside a paired grid; 8192: 32 workgroups; 4352: 17 workgroups, pairing
# switches itself off; 65536: the full 256-workgroup grid, two tiles per wave -- each phase takes its tile loop's back-edge
@pytest.mark.parametrize("n", [4096, 4091, 8192, 4352, 65536])
def test_paired_launch_equals_the_two_single_net_launches(n):
    dev = torch.device("cuda")
    up = _updater(dev)
    batch = _batch(n, n, dev)
    both, single = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    up.fp.grad.fill_(9.0)
    up._fused_loss_grad(*batch, 0.5, both)
    torch.cuda.synchronize()
    g_both = up.fp.grad.clone()
    up.fp.grad.fill_(7.0)
    up._fused_loss_grad_net(0, *batch, 0.5, single)
    up._fused_loss_grad_net(1, *batch, 0.5, single)
    torch.cuda.synchronize()
    assert torch.isfinite(g_both).all() and g_both.abs().max().item() > 0.0
    assert torch.equal(g_both, up.fp.grad)
    assert torch.equal(both, single) and both[0].item() != 0.0 and both[4].item() != 0.0


@pytest.fixture(scope="module")
def unpaired_lib():
    """the product library with csrc/ppo_mlp64.hip compiled under -DX3S_PAIR=0, bound like navbot_ppo_amd._native binds the product's"""
    tool = os.path.join(REPO, "tools", "build_mlp64_variant.py")
    try:
        r = subprocess.run([sys.executable, tool, "pair0", "-DX3S_PAIR=0"], capture_output=True, text=True)
    except OSError as e:
        pytest.skip(f"tools/build_mlp64_variant.py cannot run: {e}")
    if r.returncode != 0:
        pytest.skip("tools/build_mlp64_variant.py could not build the -DX3S_PAIR=0 library: " + r.stderr[-300:])
    L = C.CDLL(r.stdout.split()[-1])
    for name, res, args in _native.SYMBOLS:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    assert L.navsim_version() == _native.NAVSIM_ABI_VERSION
    return L


def test_update_epoch_equals_the_unpaired_build(unpaired_lib, monkeypatch):
    dev = torch.device("cuda")
    batch = _batch(8192, 5, dev)
    res = []
    for variant in (False, True):
        with monkeypatch.context() as mp:
            if variant:
                mp.setattr(_native, "lib", lambda: unpaired_lib)   # (where the entry points are called from)
            up = _updater(dev)
            up._ws.zero_()   # (stats[3] / [7] of an epoch are the squared norms the PREVIOUS step left in the workspace: none here)
            st = torch.zeros(8, device=dev)
            up._fused_epoch(*batch, 0.8, st)
            torch.cuda.synchronize()
            res.append((up.fp.flat.clone(), up._adam_m.clone(), up._adam_v.clone(), up.fp.grad.clone(), st.clone()))
    assert not torch.equal(res[0][0], _updater(dev).fp.flat)   # the epoch stepped
    for paired, unpaired in zip(*res):
        assert torch.equal(paired, unpaired)
