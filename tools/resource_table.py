"""Before / after table of the compiler's resource report (-Rpass-analysis=kernel-resource-usage) for the fused kernels.

    make -C audio-denoising_amd/csrc HIPCC="hipcc -Rpass-analysis=kernel-resource-usage" > before.log 2>&1     (on the parent commit)
    make -C audio-denoising_amd/csrc HIPCC="hipcc -Rpass-analysis=kernel-resource-usage" > after.log 2>&1      (on the change)
    python tools/resource_table.py before.log after.log [kernel name ...]

A kernel template that gained a trailing boolean parameter is matched to its old self when that parameter is false; instantiations with it true are
listed as new.  Exit status 1 when a matched kernel changed its VGPRs, AGPRs, scratch, occupancy or VGPR spills."""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "TotalSGPRs", "SGPRs Spill", "LDS Size [bytes/block]")
GATE = FIELDS[:5]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]+?): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = int(m.group(2))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"^void |\(.*$", "", d): out[n] for n, d in zip(names, dem)}


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    want = sys.argv[3:] or ["group_kernel", "hop_kernel", "frame_kernel", "sess_frame_kernel", "sess_front_kernel", "clip_analysis_kernel"]
    rows, changed = [], 0
    for name in sorted(after):
        if not any(name.startswith("dn::" + w + "<") for w in want):
            continue
        old = before.get(name)
        tag = "same name"
        if old is None and name.endswith(", false>"):
            old, tag = before.get(name[:-len(", false>")] + ">"), "default mode"
        if old is None:
            tag = "new (input phase)" if name.endswith(", true>") else "new"
        a = after[name]
        cell = lambda f: f"{old[f]}->{a[f]}" if old is not None and old.get(f) != a.get(f) else str(a.get(f))  # noqa: E731
        if old is not None and any(old.get(f) != a.get(f) for f in GATE):
            changed += 1
        rows.append((name, tag) + tuple(cell(f) for f in FIELDS))
    head = ("kernel", "matched as", "VGPRs", "AGPRs", "scratch B/lane", "waves/SIMD", "VGPR spill", "SGPRs", "SGPR spill", "LDS B")
    width = [max(len(str(r[i])) for r in rows + [head]) for i in range(len(head))]
    for r in [head] + rows:
        print("  ".join(str(c).ljust(w) for c, w in zip(r, width)))
    print(f"\n{len(rows)} kernels; {changed} matched kernels changed VGPRs, AGPRs, scratch, occupancy or VGPR spills (a->b marks a change)")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
