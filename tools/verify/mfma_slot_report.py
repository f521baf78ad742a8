#!/usr/bin/env python3
"""Static slot report of a gfx950 assembly listing: for every loop of a kernel that contains MFMAs, how many instructions sit in front
of each MFMA.  One wave per SIMD hides ~6 vector instructions behind a v_mfma_f32_32x32x16_bf16 of its own stream and pays ~4 cycles
for every further one (profiles/r06_mfma_stream.txt), so the figure to watch for a hand-placed stream (csrc/ppo_mlp64_x3s.h) is

    exposed = sum over the loop's MFMAs of max(0, fillers in front of it - 6)

where the fillers are all non-MFMA instructions except s_waitcnt.  The instructions between the loop's last MFMA and its back-edge are
a gap of their own (`tail`, with its own six free places), not part of the gap in front of the first MFMA.
These are counts from a listing, not timings.

usage: mfma_slot_report.py file.s [kernel-name-substring] [--min-mfma N] [--gaps-above N]"""
import re
import sys

from mfma_hazard_lint import parse

FREE = 6


def kernel_lines(path, key=None):
    lines = open(path).read().splitlines()
    if key:
        start = [k for k, l in enumerate(lines) if l.startswith("_Z") and key in l and l.split(";")[0].rstrip().endswith(":")]
        if not start:
            raise SystemExit(f"kernel {key} not found in {path}")
        end = [k for k in range(start[0], len(lines)) if ".amdhsa_kernel" in lines[k]][0]
        lines = lines[start[0] + 1:end]
    return lines


def kind(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_accvgpr") or op.startswith("v_mov_b"):
        return "copy"
    if op.startswith("ds_"):
        return "lds"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("scratch_"):
        return "scratch"
    if op == "s_waitcnt":
        return "waitcnt"
    if op.startswith("v_"):
        return "valu"
    return "other"


def loops(lines):
    """innermost loops as (first line, last line): a label and the last backward branch to it, with no other loop inside"""
    label_at = {}
    for n, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = n
    found = {}
    for n, l in enumerate(lines):
        p = parse(l)
        if p and p[0].startswith(("s_cbranch", "s_branch")) and p[1] and p[1][0] in label_at and label_at[p[1][0]] < n:
            found[label_at[p[1][0]]] = n
    spans = sorted(found.items())
    return [(a, b) for a, b in spans if not any(a < c and d < b for c, d in spans)]


def report(path, key=None, min_mfma=8):
    """one dict per loop with at least min_mfma MFMAs, in listing order"""
    lines = kernel_lines(path, key)
    out = []
    for a, b in loops(lines):
        ins = [p for l in lines[a:b + 1] for p in [parse(l)] if p]
        kinds = [kind(op) for op, _ in ins]
        n_mfma = kinds.count("mfma")
        if n_mfma < min_mfma:
            continue
        gaps, cur = [], 0                       # gaps[i]: fillers in front of MFMA i
        for k in kinds:
            if k == "mfma":
                gaps.append(cur)
                cur = 0
            elif k != "waitcnt":
                cur += 1
        tail = cur                              # behind the last MFMA, up to the back-edge
        ops = [op for op, _ in ins if kind(op) == "mfma"]
        out.append({
            "lines": (a, b), "instructions": len(ins), "mfma": n_mfma,
            "mfma32": sum("32x32" in o for o in ops), "mfma16": sum("16x16" in o for o in ops),
            "valu": kinds.count("valu"), "copy": kinds.count("copy"), "lds": kinds.count("lds"), "s_nop": kinds.count("s_nop"),
            "scratch": kinds.count("scratch"), "fillers": gaps, "tail": tail,
            "exposed": sum(max(0, g - FREE) for g in gaps + [tail]), "empty": sum(g <= 1 for g in gaps),
        })
    return out


def registers(path, key):
    """(.amdhsa_next_free_vgpr, .amdhsa_accum_offset) of the kernel: unified registers in use, and where the AGPRs start"""
    lines = open(path).read().splitlines()
    at = [k for k, l in enumerate(lines) if ".amdhsa_kernel" in l and key in l]
    if not at:
        raise SystemExit(f"kernel {key} not found in {path}")
    vals = {}
    for l in lines[at[0]:at[0] + 80]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|accum_offset)\s+(\d+)", l)
        if m:
            vals[m.group(1)] = int(m.group(2))
    return vals.get("next_free_vgpr"), vals.get("accum_offset")


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    opt = {argv[k]: int(argv[k + 1]) for k in range(len(argv) - 1) if argv[k].startswith("--")}
    args = [a for a in args if not a.isdigit()]
    path, key = args[0], (args[1] if len(args) > 1 else None)
    above = opt.get("--gaps-above", 12)
    for k, r in enumerate(report(path, key, opt.get("--min-mfma", 8))):
        print(f"loop {k} (lines {r['lines'][0]}..{r['lines'][1]} of the kernel): {r['instructions']} instructions, {r['mfma']} MFMAs "
              f"({r['mfma32']} 32x32 + {r['mfma16']} 16x16)")
        print(f"  vector ALU {r['valu']}, copies {r['copy']}, LDS {r['lds']}, s_nop {r['s_nop']}, scratch {r['scratch']}")
        print(f"  exposed = sum max(0, fillers - {FREE}) = {r['exposed']};  slots with 0-1 fillers: {r['empty']}")
        print("  fillers in front of each MFMA: " + " ".join(str(g) for g in r["fillers"]) + f" ; tail {r['tail']}")
        print(f"  gaps above {above}: " + (", ".join(f"{g} before MFMA {i}" for i, g in enumerate(r["fillers"]) if g > above) or "none"))
    if key:
        print("registers (next_free_vgpr, accum_offset):", registers(path, key))


if __name__ == "__main__":
    main(sys.argv[1:])
