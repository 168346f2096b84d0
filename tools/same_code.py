"""Is the device code of two trees the same?  Per-unit table over every unit of the Makefile's SRC (profiles/README.md: `*_same_code.txt`).

    python tools/same_code.py <parent checkout> <this tree> [-j N] [--work DIR [--reuse-first]] [--only UNIT ...] [-v] > profiles/<name>_same_code.txt

Every unit is compiled in both trees with the compile line its own Makefile gives it (`make -n -B`: the product flags, the unit's scheduling strategy),
`-c` replaced by `--cuda-device-only -S`.  Compared per unit: the set of function symbols and of `.amdhsa_kernel` descriptors, every function's text
from its label to its `.Lfunc_end`, every descriptor block and every kernel's entry of the metadata.  Masked before the text is compared: the
`__hip_cuid_<hash>` symbol, and the number a function has within its unit where local labels and loop comments carry it (`.LBB<n>_<k>`,
`Header=BB<n>_<k>`, `.Lfunc_end<n>`; with the run of blanks before a comment, which follows the label's width) -- kernels may come in another order.
It diffs text: nothing here knows an instruction.  Cross-compiles, no GPU needed.  Exit status 1 unless every unit is identical.
-v names the functions that differ and their first differing line, on stderr."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("audio-denoising_amd", "csrc")


def compile_lines(tree):
    """unit -> argv of its product compile line, as the tree's Makefile prints it"""
    out = subprocess.run(["make", "-C", os.path.join(tree, CSRC), "-n", "-B"], check=True, capture_output=True, text=True).stdout
    lines = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and argv[argv.index("-c") + 1].endswith(".hip"):
            lines[argv[argv.index("-c") + 1]] = argv
    return lines


def listing(tree, unit, argv, dest):
    i, o = argv.index("-c"), argv.index("-o")
    cmd = [a for k, a in enumerate(argv) if k not in (i, o, o + 1)] + ["--cuda-device-only", "-S", "-o", dest]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\n{r.stderr}")
    return dest


def mask(line):
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    line = re.sub(r"\bBB\d+_(\d+)", r"BB#_\1", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", line)
    return re.sub(r"\s+;", " ;", line.rstrip())


def parse(path):
    """(functions: symbol -> text, descriptors: symbol -> block, metadata: kernel -> entry) of one listing"""
    lines = [mask(x) for x in open(path, errors="replace")]
    syms = {m.group(1) for x in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", x)] if m}
    funcs, desc, meta = {}, {}, {}

    def blocks(into, begin, end):          # (a kernel's descriptor lies inside its function's text: one pass for each kind)
        cur = None
        for x in lines:
            if cur is None:
                m = begin(x)
                cur = (m, []) if m else None
                continue
            cur[1].append(x)
            if x.strip().startswith(end):
                into[cur[0]] = "\n".join(cur[1])
                cur = None

    def label(x):
        m = re.match(r"(\S+):", x)
        return m.group(1) if m and m.group(1) in syms else None

    def descriptor(x):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", x)
        return m.group(1) if m else None

    blocks(funcs, label, ".Lfunc_end")
    blocks(desc, descriptor, ".end_amdhsa_kernel")
    lines = [x if x.startswith(" ") else x.strip() for x in lines]
    if ".amdgpu_metadata" not in lines:
        return funcs, desc, meta
    lo, hi = lines.index(".amdgpu_metadata"), lines.index(".end_amdgpu_metadata")
    entry = []
    for x in lines[lo:hi] + ["  - "]:
        if x.startswith("  - ") and entry:
            name = [m.group(1) for y in entry for m in [re.match(r"\s+\.name:\s+(\S+)", y)] if m]
            if name:
                meta[name[0]] = "\n".join(entry)
            entry = []
        if x.startswith("  - ") or entry:
            entry.append(x)
    return funcs, desc, meta


def first_diff(a, b):
    la, lb = a.split("\n"), b.split("\n")
    for k in range(max(len(la), len(lb))):
        x, y = (la[k] if k < len(la) else "<end>"), (lb[k] if k < len(lb) else "<end>")
        if x != y:
            return f"line {k}: {x.strip()!r} | {y.strip()!r}"
    return ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("-j", type=int, default=8, help="compiles at a time (at most 16)")
    ap.add_argument("--work", help="keep the listings here (<DIR>/parent, <DIR>/change) instead of a temporary directory")
    ap.add_argument("--reuse-first", action="store_true", help="with --work: take the parent's listings that are already there")
    ap.add_argument("--only", nargs="+", metavar="UNIT", help="these units alone (dn_hop.hip ...): while a helper is being shaped")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = a.work or tmp.name
    trees = {"parent": os.path.abspath(a.parent), "change": os.path.abspath(a.change)}
    cl = {k: {u: c for u, c in compile_lines(t).items() if not a.only or u in a.only} for k, t in trees.items()}
    units = sorted(set(cl["parent"]) | set(cl["change"]))
    jobs = []
    with ThreadPoolExecutor(max(1, min(a.j, 16))) as pool:
        for k, t in trees.items():
            os.makedirs(os.path.join(work, k), exist_ok=True)
            for u in cl[k]:
                dest = os.path.join(work, k, u[:-4] + ".s")
                if not (k == "parent" and a.reuse_first and os.path.exists(dest)):
                    jobs.append(pool.submit(listing, t, u, cl[k][u], dest))
        for j in jobs:
            j.result()
    print("# device code of every unit of SRC, parent commit against this change: commands and masks in tools/same_code.py")
    print("# unit, kernel descriptors parent / change, functions parent / change, symbol sets, per-function text, .amdhsa_kernel blocks and metadata entries")
    bad = 0
    for u in units:
        if u not in cl["parent"] or u not in cl["change"]:
            print(f"{u:<24} only in {'parent' if u in cl['parent'] else 'change'}")
            bad += 1
            continue
        (f0, d0, m0), (f1, d1, m1) = (parse(os.path.join(work, k, u[:-4] + ".s")) for k in ("parent", "change"))
        same_syms = set(f0) == set(f1) and set(d0) == set(d1) and set(m0) == set(m1)
        diff_f = [s for s in sorted(set(f0) & set(f1)) if f0[s] != f1[s]]
        diff_d = [s for s in sorted(set(d0) & set(d1)) if d0[s] != d1[s]] + [s for s in sorted(set(m0) & set(m1)) if m0[s] != m1[s]]
        ok = same_syms and not diff_f and not diff_d
        bad += not ok
        print(f"{u:<24} kernels {len(d0):3d} / {len(d1):3d}  functions {len(f0):3d} / {len(f1):3d}  symbols {'same' if same_syms else 'DIFFER'}  "
              f"text {'identical' if not diff_f else f'DIFFERS in {len(diff_f)}'}  descriptors+metadata {'identical' if not diff_d else f'DIFFER in {len(diff_d)}'}")
        if a.v:
            for s in sorted((set(f0) ^ set(f1)) | (set(d0) ^ set(d1))):
                print(f"    only in one: {s}", file=sys.stderr)
            for s in diff_f:
                print(f"    {u} {s}: {first_diff(f0[s], f1[s])}", file=sys.stderr)
            for s in diff_d:
                print(f"    {u} {s}: descriptor or metadata: {first_diff(d0.get(s, ''), d1.get(s, '')) or first_diff(m0.get(s, ''), m1.get(s, ''))}", file=sys.stderr)
    print("ALL IDENTICAL" if not bad else f"{bad} UNITS DIFFER")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
