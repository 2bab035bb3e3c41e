"""th_debug_sgemm_plan (csrc/gemm.hip: the host function gemm_dispatch itself launches from) without a GPU: its ABI, the coverage of the
GPU case table of tests/test_gpu_sgemm_forms.py, and every threshold of the dispatch from both sides -- a retuned constant fails a test
here by name instead of silently moving a case of the GPU suite from one kernel to another."""
import ctypes as C

import pytest

from taper_amd._lib import INCLUDE, hip, parse_header
from tests import sgemm_ref as R
from tests.sgemm_ref import EXACT, GSCALAR, GVEC, NO_REDUCE, QUAD, RAG, SCALAR, SMALL, plan


def test_hook_is_a_debug_symbol_and_checks_its_arguments():
    assert "th_debug_sgemm_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_sgemm_plan" not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    out = (C.c_int * 12)()
    ptr = C.cast(out, C.c_void_p)
    assert hip.th_debug_sgemm_plan(0, 0, 64, 128, 784, 0, 0, 0, ptr) == 0
    for bad in [(0, 0, 0, 5, 5, 0, 0, 0), (0, 0, 5, 0, 5, 0, 0, 0), (0, 0, 5, 5, -1, 0, 0, 0), (0, 0, 5, 5, 5, 2, 0, 0), (0, 0, 5, 5, 5, 0, 16, 0),
                (0, 0, 5, 5, 5, 0, 0, -4)]:
        assert hip.th_debug_sgemm_plan(*bad, ptr) != 0 and b"th_debug_sgemm_plan" in hip.th_last_error(), bad
    assert hip.th_debug_sgemm_plan(0, 0, 5, 5, 5, 0, 0, 0, None) != 0


def test_plan_invariants_over_the_sweep():
    """what any launch needs of its plan: slices that tile k, a grid without a zero dimension, 16-byte loads only where they are possible"""
    for f, c in R.reachable_forms().items():
        ta, tb, m, n, k, ao, bo, co = c
        p = plan(*c)
        ts = p["tile"]
        assert p["tiles_m"] == -(-m // ts) and p["tiles_n"] == -(-n // ts) and p["workgroups"] == p["tiles_m"] * p["tiles_n"] * p["slices"] >= 1, c
        assert p["slices"] >= 1 and p["kslice"] % (16 if ts == 16 else 32) == 0, c
        assert (p["slices"] - 1) * p["kslice"] < k <= p["slices"] * p["kslice"], c            # every slice holds some k; together all of it
        assert (p["reduce"] == NO_REDUCE) == (p["slices"] == 1), c
        assert (p["reduce"] == QUAD) == (p["slices"] > 1 and m * n % 4 == 0 and co == 0), c
        assert not p["xcd"] or (p["slices"] > 1 and ts != 16), c
        if ts == 16:
            assert p["form"] == SMALL and p["waves"] in (4, 16), c
            assert p["a_vec"] == int(not ta and ao == 0 and k % 4 == 0) and p["b_vec"] == int(bool(tb) and bo == 0 and k % 4 == 0), c
        else:
            assert p["form"] != SMALL and p["waves"] == 4 and p["a_vec"] == p["b_vec"] == int(p["form"] != GSCALAR), c
            if p["form"] != GSCALAR:      # 16-byte rows and whole quads along each operand's contiguous axis
                assert ao == 0 and bo == 0 and (m if ta else k) % 4 == 0 and (k if tb else n) % 4 == 0, c
            if p["form"] == EXACT:
                assert m % ts == 0 and n % ts == 0 and k % 32 == 0, c


def test_case_table_covers_every_reachable_form():
    """The condition of the GPU module: its case table reaches every form th_debug_sgemm_plan reports anywhere on the sweep (dimensions
    1 ... 8192 with the tile and quad edges, the k edges of every threshold, pointers on and 4 bytes off a 16-byte boundary).

    What the sweep finds (161 forms): 16-tiles in 8 (NN: a_vec on / off), 16 (NT: both), 4 (TN: neither operand k-contiguous) and 8 (TT)
    forms -- 4 / 16 waves unsplit, 16 waves only when split (k >= 2048 > 256), both reduce kernels; 64-tiles exact-DMA, guarded-vector and
    guarded-scalar and 128-tiles exact-DMA, ragged-DMA and guarded-scalar in all four layouts, each unsplit, split and split on the XCD map
    with either reduce kernel.  Proven unreachable by the hook: ragged-DMA on 64-tiles (rag_dma asks for 128); guarded-vector on 128-tiles
    outside TN (with a k-contiguous operand `vec` already implies k % 4 == 0, all that ragged-DMA asks of k; only TN, both operands m / n-
    contiguous, needs k % 32 == 0 for it and falls back to clamped float4 loads); 4 waves with K slices on 16-tiles."""
    reach, have = R.reachable_forms(), R.cases_by_form()
    missing = sorted(f for f in reach if f not in have)
    assert not missing, "forms no GPU case reaches:\n" + "\n".join(f"  {R.form_name(f)}  e.g. {reach[f]}" for f in missing)
    assert len(reach) == 161, len(reach)      # (a change of the dispatch that adds or removes a form says so here)
    assert {(f[1], f[2]) for f in reach} == {(16, SMALL), (64, EXACT), (64, GVEC), (64, GSCALAR), (128, EXACT), (128, RAG), (128, GVEC), (128, GSCALAR)}
    assert {f[0] for f in reach if f[1:3] == (128, GVEC)} == {"TN"}
    assert all(f[6] == 16 for f in reach if f[1] == 16 and f[3])
    assert all(c[4] <= 7200 for c in R.CASES)      # the exactness argument of tests/sgemm_ref.py


def _is(c, tile, form, slices=None, kslice=None, xcd=None, reduce=None, waves=None):
    p = plan(*c)
    want = dict(tile=tile, form=form, slices=slices, kslice=kslice, xcd=xcd, reduce=reduce, waves=waves)
    got = {k: p[k] for k, v in want.items() if v is not None}
    assert got == {k: v for k, v in want.items() if v is not None}, (c, p)


@pytest.mark.parametrize("lay", R.LAYOUTS, ids=R.LAYOUT_NAMES.values())
def test_named_shapes_take_the_forms_their_comments_name(lay):
    """the shapes NAMED_CASES lists by form, in every layout where the form exists"""
    ta, tb = lay
    L = R.LAYOUT_NAMES[lay]
    _is((ta, tb, 128, 8192, 32), 128, EXACT, slices=1)
    _is((ta, tb, 640, 768, 4096), 128, EXACT, slices=16, kslice=256, xcd=0, reduce=QUAD)
    _is((ta, tb, 768, 1152, 4096), 128, EXACT, slices=9, kslice=480, xcd=1, reduce=QUAD)
    _is((ta, tb, 896, 640, 7200), 128, EXACT, slices=14, kslice=544, xcd=1)
    # ragged-DMA wants whole quads along every contiguous axis: m = 129 breaks them where A is m-contiguous (TN, TT), n = 129 where B is n-contiguous
    _is((ta, tb, 129, 4096, 32), 128, GSCALAR if ta else RAG, slices=1)
    _is((ta, tb, 129, 260, 4096), 128, GSCALAR if ta else RAG, slices=16, xcd=0)
    _is((ta, tb, 129, 4096, 4096), 128, GSCALAR if ta else RAG, slices=8, kslice=512, xcd=1)
    _is((ta, tb, 132, 4096, 32), 128, RAG, slices=1)
    _is((ta, tb, 4096, 129, 32), 128, RAG if tb else GSCALAR, slices=1)
    # k % 32 != 0 (k % 4 == 0): only TN loses ragged-DMA, to the clamped float4 loads; k % 4 != 0: scalar where an operand is k-contiguous
    _is((ta, tb, 132, 4096, 36), 128, GVEC if L == "TN" else RAG, slices=1)
    _is((ta, tb, 132, 768, 2050), 128, GVEC if L == "TN" else GSCALAR, slices=8, xcd=0)
    _is((ta, tb, 132, 8192, 2050), 128, GVEC if L == "TN" else GSCALAR, slices=4, kslice=544, xcd=1)
    # a pointer 4 bytes off the boundary: scalar loads whatever the shape
    _is((ta, tb, 129, 4096, 32, 4, 0, 0), 128, GSCALAR)
    _is((ta, tb, 132, 4096, 36, 0, 4, 0), 128, GSCALAR)
    _is((ta, tb, 129, 260, 4096, 4, 0, 4), 128, GSCALAR, reduce=SCALAR)
    _is((ta, tb, 1152, 4096, 64), 64, EXACT, slices=1)
    _is((ta, tb, 64, 1152, 4096), 64, EXACT, slices=26, kslice=160, xcd=0, reduce=QUAD)      # 26 = 3 x 8 + 2: both loops of splitk_reduce4
    _is((ta, tb, 384, 640, 4096), 64, EXACT, slices=9, kslice=480, xcd=1, reduce=QUAD)
    _is((ta, tb, 768, 2052, 256), 64, GVEC, slices=1)
    _is((ta, tb, 1152, 4096, 70), 64, GVEC if L == "TN" else GSCALAR, slices=1)
    _is((ta, tb, 96, 768, 4096), 64, GVEC, slices=22, xcd=0)
    _is((ta, tb, 65, 2048, 4096), 64, GSCALAR if ta else GVEC, slices=8, kslice=512, xcd=1)
    _is((ta, tb, 1152, 4096, 64, 4, 0, 0), 64, GSCALAR, slices=1)
    _is((ta, tb, 64, 1152, 4096, 0, 4, 4), 64, GSCALAR, slices=26, reduce=SCALAR)
    _is((ta, tb, 384, 640, 4096, 4, 4, 0), 64, GSCALAR, xcd=1, reduce=QUAD)
    _is((ta, tb, 130, 1030, 4096), 64, GVEC if L == "NT" else GSCALAR, slices=11, reduce=QUAD)      # 130 * 1030 % 4 == 0, 1030 % 4 == 2
    _is((ta, tb, 130, 130, 2048), 16, SMALL, slices=1, waves=16)                                      # 81 tiles: no K slices
    _is((ta, tb, 6, 6, 2048), 16, SMALL, slices=4, kslice=512, reduce=QUAD, waves=16)
    _is((ta, tb, 2, 6, 2052), 16, SMALL, slices=4, kslice=528, reduce=QUAD, waves=16)
    _is((ta, tb, 32, 24, 2048, 0, 0, 4), 16, SMALL, slices=4, reduce=SCALAR)
    _is((ta, tb, 17, 15, 2052, 0, 4, 4), 16, SMALL, slices=4, reduce=SCALAR)      # 255 elements: scalar by m * n % 4 too
    _is((ta, tb, 24, 24, 4095), 16, SMALL, slices=7, kslice=592, waves=16)        # 592 = 37 x 16: wave 15 of a slice gets k range [kend, kend)
    _is((ta, tb, 270, 250, 260), 16, SMALL, slices=1, waves=4)                    # 272 tiles


def test_tile_grids_off_the_raster_group_and_the_xcd_count():
    """tiles_m % 8 != 0: the raster's short last group; workgroups % 8 != 0: both branches of each XCD bijection (tile-major, slice-major)"""
    for c, tile, xcd in (((0, 0, 1152, 1152, 32), 128, 0), ((0, 0, 1100, 1130, 36), 128, 0), ((0, 0, 640, 1664, 96), 128, 0),
                         ((0, 0, 641, 1540, 2052), 128, 0), ((0, 0, 768, 1152, 4096), 128, 1), ((0, 0, 896, 640, 7200), 128, 1),
                         ((0, 0, 576, 832, 2048), 64, 0), ((0, 0, 330, 832, 4096), 64, 1)):
        p = plan(*c)
        assert (p["tile"], p["xcd"]) == (tile, xcd), (c, p)
        assert p["tiles_m"] % 8 != 0, (c, p)
        assert (p["workgroups"] if xcd else p["tiles_m"] * p["tiles_n"]) % 8 != 0, (c, p)
        assert c + (0, 0, 0) in R.CASES
    assert plan(0, 0, 1152, 1152, 32)["tiles_m"] == 9 and plan(0, 0, 576, 832, 2048)["tiles_m"] == 9      # a full group AND a short one


# ------------------------------------------------------------------------------------------------ the thresholds, from both sides
def test_threshold_tile64_kz_tiles_384():
    """tile64_kz: no K slices from 384 tiles (64 x 24512: 383, a prime; 64 x 24576: 384).  tile128_kz's `tiles >= 384` decides no launch:
    above 256 tiles 512 / tiles is one slice anyway, and a product of 257 ... 459 128-tiles deep enough to split (k >= 512) has the work for
    64-tiles and fewer than 460 workgroups, so it never reaches the 128-tile kernel (asserted at the ends of that range)"""
    _is((0, 1, 64, 24512, 512), 64, EXACT, slices=2, kslice=256)
    _is((0, 1, 64, 24576, 512), 64, EXACT, slices=1)
    _is((0, 1, 128, 128 * 256, 4096), 128, EXACT, slices=2)
    for t in (257, 383, 384, 459):
        for k in (512, 4096):
            _is((0, 1, 128, 128 * t, k), 64, EXACT, slices=1)
    _is((0, 1, 128, 128 * 460, 4096), 128, EXACT, slices=1)


def test_threshold_tile128_kz_k_512():
    """tile128_kz: K slices from k = 512 (two of 256).  At 2048 x 2048 (256 tiles) k = 511 leaves 256 workgroups < 460: the 64-tile kernel"""
    _is((0, 1, 2048, 2048, 512), 128, EXACT, slices=2, kslice=256)
    _is((0, 1, 2048, 2048, 511), 64, GSCALAR, slices=1)
    _is((0, 1, 2048, 2048, 480), 64, EXACT, slices=1)


def test_threshold_tile64_kz_k_256():
    _is((0, 1, 1216, 1024, 256), 64, EXACT, slices=2, kslice=128)
    _is((0, 1, 1216, 1024, 255), 64, GSCALAR, slices=1)
    _is((0, 1, 1216, 1024, 252), 64, GVEC, slices=1)


def test_threshold_wg128_460():
    """gemm_tile_class: a product with enough work for 64-tiles keeps the 128-tile kernel from 460 workgroups (20 x 23 tiles; 17 x 27 = 459)"""
    _is((0, 1, 2560, 2944, 64), 128, EXACT, slices=1)
    assert plan(0, 1, 2560, 2944, 64)["workgroups"] == 460
    _is((0, 1, 2176, 3456, 64), 64, EXACT, slices=1)
    assert plan(0, 1, 2176, 3456, 64)["workgroups"] == 4 * 459


def test_threshold_mid_3e8_multiply_adds():
    """gemm_is_mid: 1000 x 1000 x 300 = 3e8 multiply-adds exactly"""
    _is((0, 1, 1000, 1000, 300), 64, GVEC, slices=2)
    _is((0, 1, 1000, 1000, 299), 128, GSCALAR, slices=1)
    _is((0, 1, 1000, 1000, 296), 128, RAG, slices=1)


def test_threshold_small_slices_64_tiles_k_2048():
    """16-tiles: K slices below 64 tiles (7 x 9 = 63; 8 x 8) from k = 2048, of at least 512 k"""
    _is((0, 1, 112, 144, 2048), 16, SMALL, slices=4, kslice=512, waves=16)
    _is((0, 1, 128, 128, 2048), 16, SMALL, slices=1, waves=16)
    _is((0, 1, 112, 144, 2047), 16, SMALL, slices=1, waves=16)
    _is((0, 1, 16, 16, 4096), 16, SMALL, slices=8, kslice=512)       # k / 512 caps the 256 asked for


def test_threshold_small_wide_256_tiles_k_256():
    """16-tiles: 16 waves a workgroup below 256 tiles (15 x 17 = 255; 16 x 16) from k = 256"""
    _is((0, 1, 240, 272, 256), 16, SMALL, slices=1, waves=16)
    _is((0, 1, 256, 256, 256), 16, SMALL, slices=1, waves=4)
    _is((0, 1, 240, 272, 255), 16, SMALL, slices=1, waves=4)


@pytest.mark.parametrize("m,n,tile", [(768, 1152, 128), (384, 640, 64)])
def test_threshold_xcd_map_14_chunks(m, n, tile):
    """a split launch hands slices to the XCDs one by one from 14 chunks of 32 k a slice (9 slices of 448 / of 416)"""
    _is((0, 1, m, n, 9 * 448), tile, EXACT, slices=9, kslice=448, xcd=1)
    _is((0, 1, m, n, 9 * 416), tile, EXACT, slices=9, kslice=416, xcd=0)


def test_k0_is_one_empty_slice():
    """k == 0: 16-tiles, one slice of nothing -- no division by zero on the host, no zero in the grid (the epilogue alone: C = beta C + bias)"""
    for ta, tb in R.LAYOUTS:
        for m, n in ((5, 7), (3, 5), (1, 1), (300, 4100)):
            p = plan(ta, tb, m, n, 0)
            assert (p["tile"], p["form"], p["waves"], p["slices"], p["reduce"]) == (16, SMALL, 4, 1, NO_REDUCE) and p["kslice"] > 0, p
            assert p["workgroups"] == p["tiles_m"] * p["tiles_n"] == -(-m // 16) * -(-n // 16)
