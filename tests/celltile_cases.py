"""Cases and checks of the conv-tile comparison (tests/test_emu_celltiles.py, tests/test_gpu_celltiles.py): the stand-alone fp32 forward
(dn_cell_forward: whole row tiles on the matrix cores, the rows of a partial last row tile as fmaf chains on VALU lanes, item geometry from
compares) against the same forward on the tiles as they were (dn_cell_forward_parent_tiles), bit for bit on `out` and `hx`, with the synthetic
weights of oracle/synth_weights.py.  TEST INFRASTRUCTURE.

Shapes: the smallest at which the new tiles can go wrong.

    C  T   what it exercises
    1  1   lout = 1 at the deepest level: both edges in one item, a lone item in a tile, a single VALU-row lane
    4  3   64 mels, the compile-time C = 4 instantiation
    5  3   the product
    5  4   a second chunk of one step: the chunk boundary and tt = 1
    5  7   two full chunks and a short one

One more case at the product's shape has an inf in the input and one a NaN: there the two paths must agree in which outputs are non-finite
(and in every finite one, bit for bit).  A VALU row takes the zero-weight pad slots of its k-steps like the MFMA lanes do, so 0 x inf = NaN
appears in both or in neither.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from oracle import synth_weights

Case = namedtuple("Case", "id C T poison")
SHAPES = [(1, 1), (4, 3), (5, 3), (5, 4), (5, 7)]
CASES = [Case(f"C{c}_T{t}", c, t, None) for c, t in SHAPES] + [Case("C5_T3_inf", 5, 3, np.inf), Case("C5_T3_nan", 5, 3, np.nan)]
IDS = [c.id for c in CASES]


def inputs(case, B):
    """x (B, T, 16 C) of log-mel size, a non-zero hx (B, 17, C); the poisoned cases carry their value in one bin of the first step of stream 0
    (an interior bin: it reaches both taps of its neighbours)"""
    rng = np.random.default_rng(1000 * case.C + case.T)
    x = (2.0 * rng.standard_normal((B, case.T, 16 * case.C))).astype(np.float32)
    hx = (0.5 * rng.standard_normal((B, 17, case.C))).astype(np.float32)
    if case.poison is not None:
        x[0, 0, 37] = case.poison
    return x, hx


def bind(lib):
    """the comparison entry is not part of the public header (nor of _lib.SYMBOLS): declared in csrc/dn_internal.hpp"""
    f = lib.lib.dn_cell_forward_parent_tiles
    i32, p = C.c_int32, C.c_void_p
    f.argtypes = [p, p, p, p, p, i32, i32, i32, i32, p]
    return f


def run_both(abi, case, B):
    """-> ((out, hx) of dn_cell_forward, (out, hx) of dn_cell_forward_parent_tiles) on the same model and inputs"""
    lib = abi.lib
    parent = bind(lib)
    x, hx0 = inputs(case, B)
    m = abi.model(synth_weights.gruunet2_blob(7 + case.C), case.C)
    xd, hd = abi.up(x), abi.up(hx0)
    res = []
    for fn in (lib.dn_cell_forward, parent):
        out, hx1 = abi.nan(B, case.T, 16 * case.C), abi.nan(B, 17, case.C)
        lib.check(fn(m, abi.ptr(xd), abi.ptr(hd), abi.ptr(out), abi.ptr(hx1), B, case.T, 16 * case.C, case.C, None))
        res.append((abi.down(out), abi.down(hx1)))
    lib.dn_model_destroy(m)
    return res


def same_bits(a, b):
    """bit for bit; where a value is not finite: the same kind (NaN, +inf, -inf) in the same place"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    fin = np.isfinite(a)
    if not np.array_equal(fin, np.isfinite(b)) or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    inf = np.isinf(a)
    return np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32)) and np.array_equal(a[inf], b[inf])


def check(abi, case, B):
    (out, hx), (out_p, hx_p) = run_both(abi, case, B)
    n_bad = int((~np.isfinite(out_p)).sum()) + int((~np.isfinite(hx_p)).sum())
    diff = int((out.view(np.uint32) != out_p.view(np.uint32)).sum()) + int((hx.view(np.uint32) != hx_p.view(np.uint32)).sum())
    print(f"celltiles {case.id} B={B}: words that differ {diff}, non-finite values (parent tiles) {n_bad}, max |out| "
          f"{np.nanmax(np.abs(np.where(np.isfinite(out_p), out_p, np.nan))):.3f}")
    if case.poison is None:
        assert n_bad == 0 and np.abs(out_p).max() > 1e-3 and np.abs(hx_p).max() > 1e-3          # (a real forward, not zeros)
    # (a poisoned case may well end all finite: relu is fmaxf(., 0), which answers 0 for a NaN, so a NaN dies at the first level it meets and
    # only an inf that survives as +inf travels on; what is asked is that both paths end the same)
    assert same_bits(out, out_p) and same_bits(hx, hx_p)
