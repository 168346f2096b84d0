#!/usr/bin/env python3
"""Every ratio behind the constants model_cases.R of the synthetic-weight model tests (tests/test_emu_model_synth.py,
tests/test_gpu_model_synth.py): runs each case of tests/model_cases.py on one tier and prints, per case, the kernel's max-abs error against
float64, the fp32 CPU oracle's own error e_ref and their ratio; per family the worst ratio, the worst e_ref, the factor the rule gives
(10 x worst ratio, rounded up to a power of two) and the one the 1e-5 cap leaves.

    python tools/model_synth_margins.py --tier emu        host emulation of the kernel sources (no GPU)
    python tools/model_synth_margins.py --tier gpu        the built library on cuda:0
    python tools/model_synth_margins.py --seeds           the seed tables GRU_SEED_K, BF16_SEED_K, MOMO_SEED_K, derived again

profiles/model_synth_margins.txt is the output of both.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "emu")):
    sys.path.insert(0, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tier", choices=("emu", "gpu"))
    ap.add_argument("--seeds", action="store_true", help="derive the per-case seed tables of tests/model_cases.py again and print them")
    args = ap.parse_args()
    tier = args.tier
    import model_abi
    import model_cases as mc
    if args.seeds:
        for name, table in zip(("GRU_SEED_K", "BF16_SEED_K", "MOMO_SEED_K"), mc.derive_seed_tables()):
            print(f"{name} = {table}" + ("" if table == getattr(mc, name) else f"      # model_cases.py holds {getattr(mc, name)}"))
    if tier is None:
        return
    if tier == "emu":
        import emu
        backend, gru_modes, bf16_modes, vias = model_abi.Abi(emu.load()), ("fp32",), ("bf16",), ("abi",)
    else:
        backend, gru_modes, bf16_modes, vias = model_abi.GpuBackend(), ("fp32", "module"), ("bf16", "module-bf16"), ("abi", "module")
    rep = []
    for c in mc.GRU_CASES:
        mc.check_gru(backend, c, tier, modes=gru_modes, report=rep)
    mc.check_gru_ex(backend, tier, report=rep)
    for c in mc.GRU_BF16_CASES:
        mc.check_gru_bf16(backend, c, tier, modes=bf16_modes, report=rep)
    for g in mc.HOP_GEOMETRIES:
        mc.check_hop(backend, *g, tier, report=rep)
    for path in mc.CHAIN_PATHS:
        mc.check_chain(backend, path, tier, report=rep)
    for c in mc.MOMO_CASES:
        mc.check_momo(backend, c, tier, vias=vias, report=rep)
    print(f"# tier {tier}: max-abs error against float64 (out / residual and hx), e_ref = the fp32 CPU oracle's own, ratio = error / e_ref")
    for fam, what, err, e_ref in rep:
        print(f"{fam:7s} {what:58s} error {err:.3e}  e_ref {e_ref:.3e}  ratio {err / e_ref:7.2f}")
    print(f"# tier {tier}: per family -- worst ratio, worst e_ref, rule = 10 x worst ratio rounded up to a power of two, capped = the largest "
          f"power of two <= rule with R x e_ref <= {mc.CAP:.0e} on every case (bf16 is not capped), R in use, worst R x e_ref")
    for fam in ("gru", "gru_ex", "bf16", "hop", "momo"):
        rows = [(err / e_ref, e_ref) for f, _, err, e_ref in rep if f == fam]
        worst, e_max = max(r for r, _ in rows), max(e for _, e in rows)
        rule = mc.guard_factor(worst)
        capped = rule if fam == "bf16" else mc.capped_factor(worst, e_max)
        used = mc.R[tier][fam]
        print(f"{fam:7s} cases {len(rows):3d}  worst ratio {worst:7.2f}  worst e_ref {e_max:.3e}  rule {rule:5d}  capped {capped:5d}  "
              f"in use {used}  worst R x e_ref {used * e_max:.2e}")


if __name__ == "__main__":
    main()
