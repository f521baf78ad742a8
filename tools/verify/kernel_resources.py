"""Per-kernel resources of csrc/navsim.hip as the gfx950 code object's metadata states them, and the difference between two builds.

    python tools/verify/kernel_resources.py listing   [SRC] OUT.s      # hipcc -S --cuda-device-only with the product's flags
    python tools/verify/kernel_resources.py table     A.s              # name, VGPRs, SGPRs, scratch, LDS, kernarg bytes
    python tools/verify/kernel_resources.py compare   PARENT.s THIS.s  # both tables and their difference

`compare` is how a change that must leave the existing kernels alone shows it without a GPU: every kernel symbol of PARENT must
exist in THIS with the same VGPR / SGPR / scratch / LDS figures (the kernarg size is listed, and may differ when the parameter block
grows); kernels only THIS has are listed as new.  A kernel template that gained trailing DEFAULTED template parameters or trailing
arguments has new symbols for its old instantiations: those are paired (listed as EXTENDED) and compared like the rest.  Exit status 1 if a figure other than the kernarg size differs or a symbol is gone.
No GPU needed (hipcc cross-compiles)."""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("lds", ".group_segment_fixed_size"), ("kernarg", ".kernarg_segment_size"))


def listing(src, out):
    from navbot_ppo_amd import build
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + build.per_source_flags("navsim.hip")
    subprocess.check_call([build.hipcc()] + flags + ["-I", build.INC, "-I", os.path.join(build.HERE, "csrc"), "-S", "--cuda-device-only",
                                                    src, "-o", out])


def table(path):
    """{demangled kernel name: {field: int}} from the amdhsa.kernels metadata at the end of a listing"""
    txt = open(path).read()
    meta = txt[txt.rindex("amdhsa.kernels:"):]
    out = {}
    for blk in ("\n" + meta.split("\n", 1)[1]).split("\n  - ")[1:]:   # the top-level list items: one per kernel
        name = re.search(r"(?:^|\n)\s*\.name:\s+(\S+)", blk)
        if not name:
            continue
        row = {}
        for key, tag in FIELDS:
            m = re.search(r"(?:^|\n)\s*" + re.escape(tag) + r":\s+(\d+)", blk)
            row[key] = int(m.group(1)) if m else 0
        out[name.group(1)] = row
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n") if names else []
    short = lambda s: s.replace("(anonymous namespace)::", "")
    return {short(d) if d else n: out[n] for n, d in zip(names, dem)}


def fmt(name, r):
    return f"{name:<96} vgpr {r['vgpr']:>3} agpr {r['agpr']:>3} sgpr {r['sgpr']:>3} scratch {r['scratch']:>4} lds {r['lds']:>6} kernarg {r['kernarg']:>4}"


def _split_name(name):
    """'void f<a, b>(p, q)' -> ('f', ['a', 'b'], ['p', 'q']); the kernels' arguments hold no nested parentheses or angle brackets"""
    m = re.match(r"(?:void )?([\w:]+)(?:<([^<>]*)>)?\((.*)\)$", name)
    if not m:
        return None
    lst = lambda s: [x.strip() for x in s.split(",")] if s else []
    return m.group(1), lst(m.group(2)), lst(m.group(3))


def extended(ta, tb):
    """{parent symbol: symbol of this build} for the parent's kernels whose symbol is gone because the kernel GAINED trailing template
    parameters and / or trailing arguments (a defaulted `template <..., bool NEW = false>` changes the mangled name of every
    instantiation): the one new symbol of the same function whose template arguments start with the parent's and end in `false` / 0
    (the default) and whose argument list starts with the parent's."""
    out = {}
    for n in set(ta) - set(tb):
        pa = _split_name(n)
        if not pa:
            continue
        hits = []
        for cand in set(tb) - set(ta):
            pb = _split_name(cand)
            if (pb and pb[0] == pa[0] and pb[1][:len(pa[1])] == pa[1] and pb[2][:len(pa[2])] == pa[2]
                    and all(x in ("false", "0") for x in pb[1][len(pa[1]):])):
                hits.append(cand)
        if len(hits) == 1:
            out[n] = hits[0]
    return out


def compare(a, b):
    ta, tb = table(a), table(b)
    ext = extended(ta, tb)
    if ext:
        print("== kernels that gained defaulted template parameters / trailing arguments: compared under the parent's symbol")
        for n in sorted(ext):
            print(f"EXTENDED {n}\n      -> {ext[n]}")
            tb[n] = tb.pop(ext[n])
        print()
    bad = 0
    print(f"== parent: {len(ta)} kernels")
    for n in sorted(ta):
        print(fmt(n, ta[n]))
    print(f"\n== this build: {len(tb)} kernels")
    for n in sorted(tb):
        print(fmt(n, tb[n]))
    print("\n== difference (parent -> this build), every kernel symbol of the parent")
    same = karg = 0
    for n in sorted(ta):
        if n not in tb:
            print(f"GONE     {n}")
            bad += 1
            continue
        d = {k: (ta[n][k], tb[n][k]) for k, _ in FIELDS if ta[n][k] != tb[n][k]}
        if not d:
            same += 1
        elif set(d) == {"kernarg"}:
            karg += 1
        else:
            bad += 1
            print(f"DIFFERS  {n}: " + ", ".join(f"{k} {u} -> {v}" for k, (u, v) in d.items()))
    kd = sorted({(ta[n]["kernarg"], tb[n]["kernarg"]) for n in ta if n in tb and ta[n]["kernarg"] != tb[n]["kernarg"]})
    print(f"{same} kernels identical in every figure; {karg} differ in the kernarg size only "
          f"({', '.join(f'{u} -> {v}' for u, v in kd)}); {bad} differ otherwise or are gone")
    print("\n== new kernels")
    for n in sorted(set(tb) - set(ta)):
        print(fmt(n, tb[n]))
    return 1 if bad else 0


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "listing":
        src = sys.argv[2] if len(sys.argv) > 3 else os.path.join(REPO, "navbot_ppo_amd", "csrc", "navsim.hip")
        listing(src, sys.argv[-1])
    elif cmd == "table":
        for n, r in sorted(table(sys.argv[2]).items()):
            print(fmt(n, r))
    elif cmd == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
