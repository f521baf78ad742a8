"""The heads block of the split-bf16 update stream (csrc/ppo_mlp64_x3s.h) as the listing shows it.  F2 ends with c2[0]'s nine products and
then c2[1]'s, so that relu2 of c2[0] and its half of the heads' dot products ride behind c2[1]'s MFMAs; c2[1]'s half rides on G1's first
eight.  What is left in front of the tile's 57th MFMA (position 56: the end of the dot products, the loss arithmetic and the first two
values of dH2) was 268 instructions in the actor's loop and 74 in the critic's; the work that moved was 56 / 36 instructions, all of it
exposed before.  tools/verify/mfma_slot_report.py counts; the bounds carry the 5 % of slack of tests/test_isa_schedule_cpu.py (another
hipcc may place a few copies differently).  No GPU needed (hipcc cross-compiles)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools", "verify"))

KEY = "mlp64_pass_both_x3sE"
SLACK = 1.05
HEADS = 56                                        # G1 is 48..83: its first eight carry c2[1]'s relu and dot products
HEADS_GAP = {"actor": 215, "critic": 40}          # fillers[56]: was 268 / 74
EXPOSED = {"actor": 546 - 56, "critic": 274 - 36}  # the schedule test's counts less what moved behind F2's tail


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from navbot_ppo_amd import build
    out = tmp_path_factory.mktemp("isa_heads") / "ppo_mlp64.s"
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.hipcc()] + flags + ["-I", build.INC, "-I", os.path.join(build.HERE, "csrc"), "-S", "--cuda-device-only",
                                                    os.path.join(build.HERE, "csrc", "ppo_mlp64.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return str(out)


def test_heads_block_rides_behind_f2_tail_and_g1(listing):
    from mfma_slot_report import registers, report
    loops = [r for r in report(listing, KEY) if r["mfma"] >= 100]
    assert len(loops) == 2, [r["mfma"] for r in report(listing, KEY)]            # the actor's and the critic's tile loop, in this order
    for name, r in zip(("actor", "critic"), loops):
        print(name, "fillers[56]", r["fillers"][HEADS], "exposed", r["exposed"], "copies", r["copy"], "F2 tail", r["fillers"][30:48],
              "G1 head", r["fillers"][48:57])
        assert (r["mfma32"], r["mfma16"]) == (156, 36), (name, r["mfma32"], r["mfma16"])
        assert r["scratch"] == 0, (name, r["scratch"])
        assert r["fillers"][HEADS] <= HEADS_GAP[name] * SLACK, (name, r["fillers"][HEADS])
        assert r["exposed"] <= EXPOSED[name] * SLACK, (name, r["exposed"])
    vgpr, accum = registers(listing, KEY)
    assert accum <= 256 and vgpr - accum <= 256, (vgpr, accum)
