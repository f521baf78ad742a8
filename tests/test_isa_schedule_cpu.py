"""The schedule of the split-bf16 update stream (csrc/ppo_mlp64_x3s.h) as the listing shows it: one wave per SIMD hides about six vector
instructions behind each MFMA of its own stream and pays about four cycles for every further one (profiles/r06_mfma_stream.txt), so
what the stream costs is decided by how many instructions sit in front of each MFMA.  tools/verify/mfma_slot_report.py counts them;
this test holds the counts where the pipelined layer 1 put them (profiles/x3s_pipeline_slots.txt), so that an edit -- or a hipcc that
orders the stream differently, spills, or copies accumulators around again -- fails here.  No GPU needed (hipcc cross-compiles)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools", "verify"))

KEY = "mlp64_pass_both_x3sE"
# exposed = sum over a tile loop's MFMAs of max(0, instructions in front of it - 6).  The stream before layer 1 ran a tile ahead had
# 865 (actor loop) / 595 (critic loop); this one has 546 / 274.  5 % of slack: another hipcc may place a few copies differently.
EXPOSED = {"actor": 546, "critic": 274}
SLACK = 1.05
# positions in a tile's 192 MFMAs: F2 0..47, G1 48..83 (the heads, dH2 and the split of dH2's k-step 0 behind it), B2 84..131,
# G2 132..167, F1 of the next tile 168..179, G2 180..191
F2_FIRST, B2_FIRST, G2_FIRST, F1_FIRST = 0, 84, 132, 168


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from navbot_ppo_amd import build
    out = tmp_path_factory.mktemp("isa") / "ppo_mlp64.s"
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.hipcc()] + flags + ["-I", build.INC, "-I", os.path.join(build.HERE, "csrc"), "-S", "--cuda-device-only",
                                                    os.path.join(build.HERE, "csrc", "ppo_mlp64.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    return str(out)


def test_tile_loops_of_the_split_bf16_stream(listing):
    from mfma_slot_report import registers, report
    loops = [r for r in report(listing, KEY) if r["mfma"] >= 100]
    assert len(loops) == 2, [r["mfma"] for r in report(listing, KEY)]            # the actor's and the critic's tile loop, in this order
    for name, r in zip(("actor", "critic"), loops):
        print(name, r["instructions"], "instructions, exposed", r["exposed"], "copies", r["copy"], "fillers", r["fillers"], "tail", r["tail"])
        assert (r["mfma32"], r["mfma16"]) == (156, 36), (name, r["mfma32"], r["mfma16"])
        assert r["scratch"] == 0, (name, r["scratch"])
        assert r["exposed"] <= EXPOSED[name] * SLACK, (name, r["exposed"])
        # layer 1 runs a tile ahead: nothing is left in front of F2 or F1, and the relu mask of layer 1 no longer waits in front of G2
        # (it was 107 instructions)
        assert r["fillers"][F2_FIRST] <= 12 and r["tail"] <= 12, (name, r["fillers"][F2_FIRST], r["tail"])
        assert r["fillers"][F1_FIRST] <= 12, (name, r["fillers"][F1_FIRST])
        assert r["fillers"][G2_FIRST] <= 53, (name, r["fillers"][G2_FIRST])
        assert r["fillers"][B2_FIRST] <= 12, (name, r["fillers"][B2_FIRST])
    vgpr, accum = registers(listing, KEY)
    assert accum <= 256 and vgpr - accum <= 256, (vgpr, accum)


def test_slot_report_counts_a_small_loop(tmp_path):
    from mfma_slot_report import report
    src = tmp_path / "k.s"
    body = ["\tv_mfma_f32_32x32x16_bf16 v[16:31], a[0:3], v[4:7], v[16:31]"] * 2
    body += ["\tv_add_f32_e32 v1, v1, v2"] * 9 + ["\ts_waitcnt lgkmcnt(0)", "\tds_read_b128 a[0:3], v3", "\tv_accvgpr_mov_b32 a4, a5"]
    body += ["\tv_mfma_f32_16x16x32_bf16 a[40:43], a[0:3], a[4:7], a[40:43]", "\ts_nop 0", "\tscratch_load_dword v1, off, off"]
    src.write_text("\n".join(["_Zk:", "\tv_mov_b32_e32 v7, v9", ".LBB0_1:", "\ts_add_u32 s0, s0, 1"] + body +
                             ["\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm", "\t.amdhsa_kernel _Zk"]))
    (r,) = report(str(src), "_Zk", min_mfma=1)
    assert (r["mfma"], r["mfma32"], r["mfma16"]) == (3, 2, 1)
    assert r["fillers"] == [1, 0, 11] and r["tail"] == 3            # s_waitcnt is not counted; the back-edge branch is
    assert r["exposed"] == 5 and (r["valu"], r["copy"], r["lds"], r["s_nop"], r["scratch"]) == (9, 1, 1, 1, 1)
