"""Per-kernel ISA comparison of two source trees, or of two sets of .s files (cross-compiles, no GPU):
    python scripts/kernel_isa_diff.py TREE_A TREE_B query query_filtered ... [--filter TEXT] [-j N]
    python scripts/kernel_isa_diff.py DIR_A DIR_B query ...          (DIR_x/query.s exist: not compiled)
TREE_x is a repository root (its ggnn_amd/csrc/<unit>.hip is compiled device-only to
TREE_x/isa_diff/<unit>.s -- the directory is ignored by git) or a directory of .s files.  Kernels are
matched by mangled name; labels (.LBB / .Ltmp) and comments are normalised away.  Per kernel:
  identical   same instruction text
  reordered   same length and same multiset of opcodes, in another order (or other operands)
  different   anything else, with the instruction-count delta
and the NumVgprs / NumAgprs / ScratchSize / Occupancy / LDSByteSize / spill counts of both sides where
they differ.  Exit status 1 if the kernel sets differ or a kernel of B has a larger private segment,
fewer waves per SIMD, another LDS size or a spill count that A does not have."""
import argparse, collections, difflib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++20", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-S"]
INFO = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def asm_of(root, unit):
    s = os.path.join(root, unit + ".s")
    if os.path.exists(s):
        return s
    out = os.path.join(root, "isa_diff")
    os.makedirs(out, exist_ok=True)
    s = os.path.join(out, unit + ".s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", *FLAGS,
                    os.path.join(root, "ggnn_amd", "csrc", unit + ".hip"), "-o", s],
                   check=True, capture_output=True)
    return s


def kernels_of(path):
    """{mangled name: (instructions, {info key: int})}"""
    out, name, body = {}, None, None
    spills = {}
    text = open(path).read()
    for blk in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):]):
        n = re.search(r"\.name:\s+(\S+)", blk)
        if n:
            spills[n.group(1)] = {k: int(v) for k, v in re.findall(r"\.((?:v|s)gpr_spill_count):\s+(\d+)", blk)}
    for line in text.splitlines():
        m = re.match(r"(_Z\w+):\s", line)
        if m and m.group(1) in spills:
            name, body = m.group(1), []
            out[name] = (body, dict(spills[name]))
            continue
        if name is None:
            continue
        if body is not None:
            t = line.split(";")[0].strip()
            if t.startswith(".Lfunc_end"):
                body = None
            elif t and not t.startswith(".") and not t.endswith(":"):
                out[name][0].append(re.sub(r"\.L(BB|tmp)[\d_]+", ".L", t))
            continue
        m = re.match(r"; (\w+): (\d+)", line)
        if m and m.group(1) in INFO:
            out[name][1][m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                name = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"), ap.add_argument("b"), ap.add_argument("units", nargs="+")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--hunks", action="store_true", help="print the diff hunks of reordered kernels")
    ap.add_argument("-j", type=int, default=4)
    o = ap.parse_args()
    with ThreadPoolExecutor(o.j) as ex:
        files = list(ex.map(lambda ru: asm_of(*ru), [(r, u) for u in o.units for r in (o.a, o.b)]))
    bad = 0
    for i, unit in enumerate(o.units):
        ka, kb = kernels_of(files[2 * i]), kernels_of(files[2 * i + 1])
        if set(ka) != set(kb):
            bad += 1
            print(f"{unit}: kernel sets differ: only A {sorted(set(ka) - set(kb))[:5]} "
                  f"only B {sorted(set(kb) - set(ka))[:5]}")
        names = sorted(set(ka) & set(kb))
        pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                                text=True).stdout.splitlines()
        count, regs = collections.Counter(), collections.Counter()
        for n, p in zip(names, pretty):
            p = re.sub(r"\(.*", "", p).replace("ggnn_amd::", "").replace("void ", "")
            (ia, ma), (ib, mb) = ka[n], kb[n]
            if ia == ib:
                kind = "identical"
            elif len(ia) == len(ib) and (collections.Counter(x.split()[0] for x in ia) ==
                                         collections.Counter(x.split()[0] for x in ib)):
                kind = "reordered"
            else:
                kind = f"different ({len(ib) - len(ia):+d} of {len(ia)})"
            count[kind.split()[0]] += 1
            worse = (mb["ScratchSize"] > ma["ScratchSize"] or mb["Occupancy"] < ma["Occupancy"] or
                     mb["LDSByteSize"] != ma["LDSByteSize"] or
                     any(mb.get(k, 0) > 0 and ma.get(k, 0) == 0 for k in ("vgpr_spill_count", "sgpr_spill_count")))
            bad += worse
            for k in ("NumVgprs", "NumAgprs"):
                if ma[k] != mb[k]:
                    regs[f"{k} {mb[k] - ma[k]:+d}"] += 1
            if o.filter not in p or (kind == "identical" and not o.filter):
                continue
            delta = " ".join(f"{k} {ma.get(k)}->{mb.get(k)}" for k in sorted(set(ma) | set(mb))
                             if ma.get(k) != mb.get(k))
            print(f"{unit}: {'WORSE ' if worse else ''}{kind:10s} {p}  [{len(ia)} instr] {delta}")
            if o.hunks and kind != "identical":
                sm = difflib.SequenceMatcher(None, ia, ib, autojunk=False)
                for tag, a0, a1, b0, b1 in sm.get_opcodes():
                    if tag != "equal":
                        print(f"    @{a0}: -{ia[a0:a1]} +{ib[b0:b1]}")
        print(f"{unit}: {len(names)} kernels: " + ", ".join(f"{v} {k}" for k, v in sorted(count.items())) +
              ("; registers: " + ", ".join(f"{v} x {k}" for k, v in sorted(regs.items())) if regs else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
