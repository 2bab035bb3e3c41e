"""Shared by tests/test_sgemm_plan.py (no GPU) and tests/test_gpu_sgemm_forms.py: th_debug_sgemm_plan as a dict, the sweep that finds every
reachable kernel form of csrc/gemm.hip, the GPU case table, and the exact reference.

A FORM is the tuple (layout, tile class, load form, split, slice-per-XCD map, reduce kernel, waves, a_vec, b_vec): what decides which
kernel instance runs and which of its paths.  The exact-arithmetic checks rest on integers: operands in [-4, 4], C0 and bias in [-8, 8];
with k <= 7200 every product, partial sum and epilogue value is a multiple of 0.5 below 2^17, so every summation order, MFMA chain and
slice order gives the same float32 bits as numpy's float64 product."""
import ctypes as C
import functools
import itertools

import numpy as np

f32 = np.float32
PLAN_FIELDS = ("tile", "form", "waves", "a_vec", "b_vec", "slices", "kslice", "workgroups", "xcd", "reduce", "tiles_m", "tiles_n")
SMALL, EXACT, RAG, GVEC, GSCALAR = range(5)                 # load forms
FORM_NAMES = ("small", "exact-DMA", "ragged-DMA", "guarded-vector", "guarded-scalar")
NO_REDUCE, QUAD, SCALAR = range(3)                          # reduce kernels: none, splitk_reduce4, splitk_reduce
REDUCE_NAMES = ("-", "splitk_reduce4", "splitk_reduce")
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))                  # (trans_a, trans_b): NN, NT, TN, TT
LAYOUT_NAMES = {(0, 0): "NN", (0, 1): "NT", (1, 0): "TN", (1, 1): "TT"}
ALPHA_BETA = ((1.0, 0.0), (1.0, 1.0), (0.5, -2.0))


def _lib():
    from taper_amd._lib import hip
    return hip


def plan(ta, tb, m, n, k, ao=0, bo=0, co=0):
    """th_debug_sgemm_plan as a dict (pure host code: no context, no device); ao / bo / co: bytes off a 16-byte boundary"""
    out = (C.c_int * 12)()
    assert _lib().th_debug_sgemm_plan(ta, tb, m, n, k, ao, bo, co, C.cast(out, C.c_void_p)) == 0, _lib().th_last_error()
    return dict(zip(PLAN_FIELDS, out))


def form_of(ta, tb, m, n, k, ao=0, bo=0, co=0):
    p = plan(ta, tb, m, n, k, ao, bo, co)
    return (LAYOUT_NAMES[(ta, tb)], p["tile"], p["form"], int(p["slices"] > 1), p["xcd"], p["reduce"], p["waves"], p["a_vec"], p["b_vec"])


def form_name(f):
    lay, tile, form, split, xcd, red, waves, av, bv = f
    return (f"{lay} {tile}-tiles {FORM_NAMES[form]}" + (" split" if split else "") + (" XCD-map" if xcd else "") +
            (f" {REDUCE_NAMES[red]}" if red else "") + (f" {waves} waves a_vec={av} b_vec={bv}" if tile == 16 else ""))


# the sweep: every dimension edge the dispatch looks at (16 / 64 / 128 tiles and quads), 1 ... 8192, and the k edges of its thresholds
SWEEP_DIMS = (1, 4, 15, 16, 17, 63, 64, 65, 96, 127, 128, 129, 130, 132, 256, 260, 384, 640, 768, 1028, 1030, 1152, 2048, 2052, 4096, 4100, 8192)
SWEEP_K = (1, 15, 16, 17, 31, 32, 36, 70, 255, 256, 260, 511, 512, 2047, 2048, 2050, 4096)
MISALIGN = (0, 4)


@functools.lru_cache(maxsize=None)
def reachable_forms():
    """{form: the smallest (ta, tb, m, n, k, ao, bo, co) of the sweep that reaches it}"""
    found = {}
    for (ta, tb), m, n, k in itertools.product(LAYOUTS, SWEEP_DIMS, SWEEP_DIMS, SWEEP_K):
        for ao, bo, co in itertools.product(MISALIGN, repeat=3):
            f = form_of(ta, tb, m, n, k, ao, bo, co)
            if f not in found or m * n * k < found[f][2] * found[f][3] * found[f][4]:
                found[f] = (ta, tb, m, n, k, ao, bo, co)
    return found


# ---------------------------------------------------------------------------------------------------------------- data and reference
def operands(case, b_nonzero=False, seed=0):
    """integer operands of a case as they lie in memory: A [m, k] ([k, m] transposed), B [k, n] ([n, k] transposed), C0 [m, n], bias [n]"""
    ta, tb, m, n, k = case[:5]
    rng = np.random.default_rng([seed, ta, tb, m, n, k])
    a = rng.integers(-4, 5, (k, m) if ta else (m, k), dtype=np.int8).astype(f32)      # mostly non-zero: one in nine is 0
    b = rng.integers(-4, 5, (n, k) if tb else (k, n), dtype=np.int8).astype(f32)
    if b_nonzero:
        b[b == 0] = 3
    c0 = rng.integers(-8, 9, (m, n)).astype(f32)
    bias = rng.integers(-8, 9, n).astype(f32)
    return a, b, c0, bias


def product64(case, a, b):
    """op(A) @ op(B) in float64: exact on these integers"""
    ta, tb = case[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)


def epilogue(prod, alpha, beta, c0=None, bias=None, relu=False):
    """the epilogue of th_sgemm / th_linear_fwd in float64, cast to float32; beta == 0 does not read C0"""
    v = alpha * prod
    if beta != 0.0:
        v = v + beta * c0.astype(np.float64)
    if bias is not None:
        v = v + bias.astype(np.float64)[None, :]
    if relu:
        v = np.where(v > 0, v, 0.0)      # (a NaN stays out of reach: v > 0 is False -> 0, as in the kernel)
    return v.astype(f32)


# ---------------------------------------------------------------------------------------------------------------- the GPU case table
# (ta, tb, m, n, k, a offset, b offset, c offset): offsets in bytes off a 16-byte boundary.  tests/test_sgemm_plan.py asserts that this table
# reaches every form of reachable_forms(); the generated part below is the smallest shape of the sweep per form.
def _all_layouts(m, n, k, ao=0, bo=0, co=0):
    return [(ta, tb, m, n, k, ao, bo, co) for ta, tb in LAYOUTS]


NAMED_CASES = (
    # ---- 128-tiles: whole tiles unsplit / split (16 slices of 256) / split on the slice-per-XCD map (9 slices of 480: the largest case)
    _all_layouts(128, 8192, 32) + _all_layouts(640, 768, 4096) + _all_layouts(768, 1152, 4096)
    # ---- 128-tiles, ragged: rows past m; quads past n; the last k chunk's quads (k % 32 = 4); TN / TT need m % 4 == 0; each one scalar by pointer
    + _all_layouts(129, 4096, 32) + _all_layouts(129, 260, 4096) + _all_layouts(129, 4096, 4096) + _all_layouts(132, 4096, 32)
    + _all_layouts(4096, 129, 32) + _all_layouts(132, 4096, 36) + _all_layouts(132, 768, 2050) + _all_layouts(132, 8192, 2050)
    + _all_layouts(129, 4096, 32, 4, 0, 0) + _all_layouts(129, 260, 4096, 4, 0, 4) + _all_layouts(132, 4096, 36, 0, 4, 0)
    # ---- 64-tiles: whole tiles unsplit / split (26 slices: splitk_reduce4's 8-slab loop three times and a remainder of 2) / XCD map
    + _all_layouts(1152, 4096, 64) + _all_layouts(64, 1152, 4096) + _all_layouts(384, 640, 4096)
    # ---- 64-tiles, guarded: quads past n; k % 32 = 6; split; split on the XCD map with a row past m; scalar by pointer alone
    + _all_layouts(768, 2052, 256) + _all_layouts(1152, 4096, 70) + _all_layouts(96, 768, 4096) + _all_layouts(65, 2048, 4096)
    + _all_layouts(1152, 4096, 64, 4, 0, 0) + _all_layouts(64, 1152, 4096, 0, 4, 4) + _all_layouts(384, 640, 4096, 4, 4, 0)
    # ---- tile grids whose row count is no multiple of the raster group (8) and whose size is no multiple of the XCD count: the short last
    #      group and both XCD bijections (unsplit / tile-major split: 9 x 9 and 5 x 13 tiles; slice-major split: 6 x 9 x 9 above, 7 x 5 x 15)
    + _all_layouts(1152, 1152, 32) + _all_layouts(1100, 1130, 36) + _all_layouts(640, 1664, 96) + _all_layouts(641, 1540, 2052)
    + _all_layouts(896, 640, 7200) + _all_layouts(576, 832, 2048) + _all_layouts(330, 832, 4096)
    # ---- split products with m * n % 4 == 0 and n % 4 != 0: a quad of splitk_reduce4 straddles two rows (th_linear_fwd: its bias index is
    #      (i + e) % n) -- on 64-tiles and on 16-tiles; 130 x 130 x 2048 has 81 16-tiles and stays unsplit on 16 waves
    + _all_layouts(130, 1030, 4096) + _all_layouts(6, 6, 2048) + _all_layouts(2, 6, 2052) + _all_layouts(130, 130, 2048)
    # ---- 16-tiles: m, n in {1, 15, 16, 17}; k no multiple of 16 / of 16 waves (waves with an empty k range); 4 and 16 waves; K slices
    + [c for m, n in ((1, 1), (15, 17), (16, 16), (17, 15), (1, 17), (16, 1)) for k in (1, 17, 36, 260, 2050) for c in _all_layouts(m, n, k)]
    + _all_layouts(33, 40, 300) + _all_layouts(270, 250, 260) + _all_layouts(100, 9, 4096) + _all_layouts(24, 24, 4095)
    # ---- 16-tiles: a_vec / b_vec switched off by pointer (k % 4 == 0) and by k % 4; the scalar reduce by C's pointer and by m * n % 4
    + _all_layouts(17, 33, 64, 4, 0, 0) + _all_layouts(17, 33, 64, 0, 4, 0) + _all_layouts(17, 33, 66) + _all_layouts(32, 24, 2048, 0, 0, 4)
    + _all_layouts(32, 24, 2048, 4, 4, 0) + _all_layouts(17, 15, 2052, 0, 4, 4)
)

# the smallest shape of the sweep for every form the named cases above do not reach (regenerate: python -m tests.sgemm_ref)
GENERATED_CASES = [
    (0, 0, 1, 1, 256, 4, 0, 0),   # NN 16-tiles small 16 waves a_vec=0 b_vec=0
    (0, 0, 64, 1152, 4096, 0, 0, 4),   # NN 64-tiles exact-DMA split splitk_reduce
    (0, 0, 384, 640, 4096, 0, 0, 4),   # NN 64-tiles exact-DMA split XCD-map splitk_reduce
    (0, 0, 96, 768, 4096, 0, 0, 4),   # NN 64-tiles guarded-vector split splitk_reduce
    (0, 0, 65, 2048, 4096, 0, 0, 4),   # NN 64-tiles guarded-vector split XCD-map splitk_reduce
    (0, 0, 768, 768, 511, 0, 0, 0),   # NN 64-tiles guarded-scalar split splitk_reduce4
    (0, 0, 65, 4096, 2047, 0, 0, 4),   # NN 64-tiles guarded-scalar split XCD-map splitk_reduce
    (0, 0, 640, 768, 4096, 0, 0, 4),   # NN 128-tiles exact-DMA split splitk_reduce
    (0, 0, 768, 1152, 4096, 0, 0, 4),   # NN 128-tiles exact-DMA split XCD-map splitk_reduce
    (0, 0, 129, 260, 4096, 0, 0, 4),   # NN 128-tiles ragged-DMA split splitk_reduce
    (0, 0, 129, 4096, 4096, 0, 0, 4),   # NN 128-tiles ragged-DMA split XCD-map splitk_reduce
    (0, 0, 129, 8192, 2047, 0, 0, 4),   # NN 128-tiles guarded-scalar split XCD-map splitk_reduce
    (0, 1, 1, 1, 256, 4, 4, 0),   # NT 16-tiles small 16 waves a_vec=0 b_vec=0
    (0, 1, 1, 1, 256, 4, 0, 0),   # NT 16-tiles small 16 waves a_vec=0 b_vec=1
    (0, 1, 1, 1, 256, 0, 4, 0),   # NT 16-tiles small 16 waves a_vec=1 b_vec=0
    (0, 1, 1, 4, 2048, 4, 0, 0),   # NT 16-tiles small split splitk_reduce4 16 waves a_vec=0 b_vec=1
    (0, 1, 1, 4, 2048, 0, 4, 0),   # NT 16-tiles small split splitk_reduce4 16 waves a_vec=1 b_vec=0
    (0, 1, 1, 1, 2048, 4, 0, 0),   # NT 16-tiles small split splitk_reduce 16 waves a_vec=0 b_vec=1
    (0, 1, 64, 1152, 4096, 0, 0, 4),   # NT 64-tiles exact-DMA split splitk_reduce
    (0, 1, 384, 640, 4096, 0, 0, 4),   # NT 64-tiles exact-DMA split XCD-map splitk_reduce
    (0, 1, 96, 768, 4096, 0, 0, 4),   # NT 64-tiles guarded-vector split splitk_reduce
    (0, 1, 65, 2048, 4096, 0, 0, 4),   # NT 64-tiles guarded-vector split XCD-map splitk_reduce
    (0, 1, 768, 768, 511, 0, 0, 0),   # NT 64-tiles guarded-scalar split splitk_reduce4
    (0, 1, 65, 4096, 2047, 0, 0, 4),   # NT 64-tiles guarded-scalar split XCD-map splitk_reduce
    (0, 1, 640, 768, 4096, 0, 0, 4),   # NT 128-tiles exact-DMA split splitk_reduce
    (0, 1, 768, 1152, 4096, 0, 0, 4),   # NT 128-tiles exact-DMA split XCD-map splitk_reduce
    (0, 1, 129, 260, 4096, 0, 0, 4),   # NT 128-tiles ragged-DMA split splitk_reduce
    (0, 1, 129, 4096, 4096, 0, 0, 4),   # NT 128-tiles ragged-DMA split XCD-map splitk_reduce
    (0, 1, 129, 8192, 2047, 0, 0, 4),   # NT 128-tiles guarded-scalar split XCD-map splitk_reduce
    (1, 0, 64, 1152, 4096, 0, 0, 4),   # TN 64-tiles exact-DMA split splitk_reduce
    (1, 0, 384, 640, 4096, 0, 0, 4),   # TN 64-tiles exact-DMA split XCD-map splitk_reduce
    (1, 0, 768, 768, 511, 0, 0, 4),   # TN 64-tiles guarded-vector split splitk_reduce
    (1, 0, 96, 4096, 2047, 0, 0, 0),   # TN 64-tiles guarded-vector split XCD-map splitk_reduce4
    (1, 0, 96, 4096, 2047, 0, 0, 4),   # TN 64-tiles guarded-vector split XCD-map splitk_reduce
    (1, 0, 768, 768, 511, 0, 4, 0),   # TN 64-tiles guarded-scalar split splitk_reduce4
    (1, 0, 65, 4096, 2047, 0, 0, 4),   # TN 64-tiles guarded-scalar split XCD-map splitk_reduce
    (1, 0, 640, 768, 4096, 0, 0, 4),   # TN 128-tiles exact-DMA split splitk_reduce
    (1, 0, 768, 1152, 4096, 0, 0, 4),   # TN 128-tiles exact-DMA split XCD-map splitk_reduce
    (1, 0, 132, 260, 4096, 0, 0, 0),   # TN 128-tiles ragged-DMA split splitk_reduce4
    (1, 0, 132, 260, 4096, 0, 0, 4),   # TN 128-tiles ragged-DMA split splitk_reduce
    (1, 0, 132, 4096, 4096, 0, 0, 0),   # TN 128-tiles ragged-DMA split XCD-map splitk_reduce4
    (1, 0, 132, 4096, 4096, 0, 0, 4),   # TN 128-tiles ragged-DMA split XCD-map splitk_reduce
    (1, 0, 132, 768, 2050, 0, 0, 4),   # TN 128-tiles guarded-vector split splitk_reduce
    (1, 0, 132, 8192, 2047, 0, 0, 4),   # TN 128-tiles guarded-vector split XCD-map splitk_reduce
    (1, 0, 129, 8192, 2047, 0, 0, 4),   # TN 128-tiles guarded-scalar split XCD-map splitk_reduce
    (1, 1, 1, 1, 256, 0, 4, 0),   # TT 16-tiles small 16 waves a_vec=0 b_vec=0
    (1, 1, 64, 1152, 4096, 0, 0, 4),   # TT 64-tiles exact-DMA split splitk_reduce
    (1, 1, 384, 640, 4096, 0, 0, 4),   # TT 64-tiles exact-DMA split XCD-map splitk_reduce
    (1, 1, 96, 768, 4096, 0, 0, 4),   # TT 64-tiles guarded-vector split splitk_reduce
    (1, 1, 2048, 65, 4096, 0, 0, 0),   # TT 64-tiles guarded-vector split XCD-map splitk_reduce4
    (1, 1, 2048, 65, 4096, 0, 0, 4),   # TT 64-tiles guarded-vector split XCD-map splitk_reduce
    (1, 1, 768, 768, 511, 0, 0, 0),   # TT 64-tiles guarded-scalar split splitk_reduce4
    (1, 1, 65, 4096, 2047, 0, 0, 4),   # TT 64-tiles guarded-scalar split XCD-map splitk_reduce
    (1, 1, 640, 768, 4096, 0, 0, 4),   # TT 128-tiles exact-DMA split splitk_reduce
    (1, 1, 768, 1152, 4096, 0, 0, 4),   # TT 128-tiles exact-DMA split XCD-map splitk_reduce
    (1, 1, 260, 129, 4096, 0, 0, 0),   # TT 128-tiles ragged-DMA split splitk_reduce4
    (1, 1, 260, 129, 4096, 0, 0, 4),   # TT 128-tiles ragged-DMA split splitk_reduce
    (1, 1, 4096, 129, 4096, 0, 0, 0),   # TT 128-tiles ragged-DMA split XCD-map splitk_reduce4
    (1, 1, 4096, 129, 4096, 0, 0, 4),   # TT 128-tiles ragged-DMA split XCD-map splitk_reduce
    (1, 1, 129, 8192, 2047, 0, 0, 4),   # TT 128-tiles guarded-scalar split XCD-map splitk_reduce
]

CASES = list(dict.fromkeys(list(NAMED_CASES) + GENERATED_CASES))


def case_id(c):
    return LAYOUT_NAMES[c[:2]] + "-" + "x".join(map(str, c[2:5])) + ("" if not any(c[5:]) else "-off" + "".join(str(o // 4) for o in c[5:]))


def cases_by_form():
    out = {}
    for c in CASES:
        out.setdefault(form_of(*c), []).append(c)
    return out


if __name__ == "__main__":      # prints what GENERATED_CASES lacks, then the table of forms of DESIGN.md section 3a
    have, reach = cases_by_form(), reachable_forms()
    for f in sorted(reach):
        if f not in have:
            print(f"    {reach[f]},   # {form_name(f)}")
    print(f"{len(reach)} forms reachable, {len(have)} reached by the case table")
    print("| tile class | load form | layouts | variants per layout | forms | smallest shape of the sweep (layout m x n x k) |\n|---|---|---|---|---|---|")
    for tile, form in sorted({f[1:3] for f in reach}):
        fs = [f for f in reach if f[1:3] == (tile, form)]
        lays = sorted({f[0] for f in fs})
        c = min((reach[f] for f in fs), key=lambda c: c[2] * c[3] * c[4])
        var = ("4 / 16 waves unsplit, 16 waves split x {splitk_reduce4, splitk_reduce}, x a_vec / b_vec where the operand is k-contiguous"
               if tile == 16 else "unsplit; split and split on the XCD map, each x {splitk_reduce4, splitk_reduce}")
        print(f"| {tile} | {FORM_NAMES[form]} | {' '.join(lays)} | {var} | {len(fs)} | {LAYOUT_NAMES[c[:2]]} {c[2]} x {c[3]} x {c[4]} |")
