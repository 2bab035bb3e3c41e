"""th_debug_conv3x3_plan (csrc/conv_plan.h: the host functions the 3x3 convolution entry points themselves launch from) without a GPU: its
ABI, the coverage of the GPU case table of tests/test_gpu_conv_forms.py, the plan's invariants over the whole sweep, the thresholds of the
dispatch from both sides -- a retuned constant fails a test here by name instead of silently moving a case of the GPU suite from one kernel
to another -- and tests/conv_ref.py's numpy reference against the oracle, on bits."""
import ctypes as C

import numpy as np
import pytest

from taper_amd._lib import INCLUDE, hip, parse_header
from tests import conv_ref as R
from tests.conv_ref import (BWD_INPUT, BWD_WEIGHT, CHAIN, CONV1, FWD, GAP, IMG, MFMA, POOL2, R_COLSUM, R_COLSUM_ACCUM, R_NONE, R_SCATTER,
                            R_SLAB_SUM, REFUSED, ROWS, TILE, WGRAD_CONV1, WGRAD_IMG, WGRAD_MFMA, WGRAD_VEC, _c, plan)


def test_hook_is_a_debug_symbol_and_checks_its_arguments():
    assert "th_debug_conv3x3_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_conv3x3_plan" not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    out = (C.c_int * len(R.PLAN_FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = (0, 4, 8, 14, 14, 16, 1, 0, 3, 0, 0, -1)
    assert hip.th_debug_conv3x3_plan(*good, ptr) == 0
    for i, v in ((0, 5), (0, -1), (1, 0), (2, 0), (3, 0), (4, -3), (5, 0), (6, 2), (6, -1), (7, 2), (8, 4), (9, 2), (10, 2), (10, 16), (11, 2), (11, -2)):
        bad = list(good)
        bad[i] = v
        assert hip.th_debug_conv3x3_plan(*bad, ptr) != 0 and b"th_debug_conv3x3_plan" in hip.th_last_error(), bad
    assert hip.th_debug_conv3x3_plan(0, 1, 1, 2, 5, 1, 0, 0, 3, 0, 0, -1, ptr) != 0 and b"bad geometry" in hip.th_last_error()      # no 3x3 window
    assert hip.th_debug_conv3x3_plan(0, 4, 8, 14, 14, 16, 1, 0, 3, 1, 0, -1, ptr) != 0      # a forward does not accumulate
    assert hip.th_debug_conv3x3_plan(*good, None) != 0
    # the struct and the field list of tests/conv_ref.py are the same length: the last field is w_out
    assert plan(*good)["w_out"] == 14 and plan(0, 1, 8, 5, 9, 4, pad=0)["h_out"] == 3


def test_plan_invariants_over_the_sweep():
    """tests/conv_ref.py: violations() on every plan of the sweep -- img_t >= 1 and rows_t * w_out <= 128, LDS at or below the limit the launch
    requests, G <= min(n_pb, 512), the in-place weight path only with c_out % 4 == 0 and an aligned pointer, gap and pool forms only in their
    ops, and the *_supported queries in agreement with the plan"""
    bad = R.sweep()[1]
    assert not bad, f"{len(bad)} broken invariants, e.g. " + "; ".join(f"{c}: {b}" for c, b in bad[:5])


def test_case_table_covers_every_reachable_form():
    """The condition of the GPU module: its case table reaches every form th_debug_conv3x3_plan reports anywhere on the sweep.

    What the sweep finds (187 forms): forward 60, pool 24, gap 9, input gradient 46, weight gradient 48.  Not reachable from the public entry
    points, by the dispatch's own conditions: conv3x3_mfma_kernel<CT = 1, ..., WH = 2> and <CT = 1, ..., DMA> (both ask for CT >= 2);
    <ACC, POOL> together (no caller accumulates into a pooled map); DMA with CIT = 1 or ACC; the image-resident and chain kernels with
    accumulate; CT = 4 with POOL below 384 workgroup slots; conv_wgrad_img_kernel and the LIN chains below 128 images."""
    reach, have = R.reachable_forms(), R.cases_by_form()
    missing = sorted(f for f in reach if f not in have)
    assert not missing, "forms no GPU case reaches:\n" + "\n".join(f"  {R.form_name(f)}  e.g. {reach[f]}" for f in missing)
    assert len(reach) == 187, len(reach)      # (a change of the dispatch that adds or removes a form says so here)
    assert [sum(1 for f in reach if f[0] == op) for op in range(5)] == [60, 24, 9, 46, 48]
    assert {f[1] for f in reach} == {REFUSED, CONV1, TILE, ROWS, MFMA, IMG, CHAIN, WGRAD_MFMA, WGRAD_IMG, WGRAD_CONV1, WGRAD_VEC}
    mf = [f for f in reach if f[1] == MFMA]
    assert all(f[2] >= 2 for f in mf if f[6] == 2 or f[7]) and not any(f[3] and (f[5] or f[7]) for f in mf) and not any(f[4] == 1 and f[7] for f in mf)
    # every case stands inside the exactness argument of tests/conv_ref.py
    for c in R.CASES:
        op, n, c_in, h, w, c_out, pad = c[:7]
        assert 16 * 9 * max(c_in, c_out) + 16 < 2 ** 24 and 16 * n * (h + 2 * pad - 2) * (w + 2 * pad - 2) + 8 < 2 ** 24, c


def _is(case, **want):
    p = plan(*case)
    assert {k: p[k] for k in want} == want, (case, R.form_name(R.form_of(*case)), p)


def test_named_rows_take_the_forms_their_comments_name():
    """the rows NAMED_CASES lists by what they are there for"""
    _is(_c(FWD, 2, 8, 14, 14, 16, img_mode=0), family=MFMA, rows_t=9, bands=2, img_t=1)                 # 14 % 9 != 0: a ragged last band
    _is(_c(FWD, 11, 9, 7, 7, 17), family=MFMA, img_t=9, dma=0, prep=1)                                  # 11 % 9 != 0, c_in % 8 != 0
    _is(_c(FWD, 1, 8, 4, 126, 4), family=MFMA, prep=0)
    _is(_c(FWD, 1, 8, 4, 127, 4), family=ROWS, px=1, prep=1)
    _is(_c(FWD, 1, 8, 6, 128, 8, pad=0), family=MFMA)                                                   # w_out = 126 without padding
    _is(_c(POOL2, 2, 8, 6, 64, 4), family=MFMA, pool=1)
    _is(_c(POOL2, 2, 8, 6, 66, 4), family=REFUSED, refused=3)
    _is(_c(FWD, 3, 1, 9, 7, 20, layout=1), family=MFMA, cit=1, prep=1)
    _is(_c(POOL2, 3, 1, 28, 28, 32), family=CONV1, pool=1)
    _is(_c(FWD, 1, 1, 110, 110, 4), family=MFMA, cit=1, prep=0)                                         # 112 x 112 x 4 B > 48 KB
    _is(_c(FWD, 1, 1, 108, 108, 4), family=CONV1)                                                       # 110 x 110 x 4 B = 48 400 B
    _is(_c(POOL2, 1, 1, 186, 64, 4), family=MFMA, cit=1, pool=1)                                        # 188 x 66 x 4 B > 48 KB
    _is(_c(POOL2, 1, 1, 110, 110, 4), family=REFUSED, refused=3)                                        # rows of more than 64 outputs
    _is(_c(FWD, 2, 3, 72, 72, 4), family=REFUSED, refused=1)
    _is(_c(BWD_INPUT, 2, 4, 72, 72, 3), family=REFUSED, refused=1)
    _is(_c(FWD, 2, 3, 69, 69, 4), family=ROWS)                                                          # 71 x 71 x 32 B = 161 312 B fits
    _is(_c(BWD_WEIGHT, 257, 8, 3, 3, 16), family=WGRAD_MFMA, pq=2)
    _is(_c(BWD_WEIGHT, 11, 8, 14, 14, 16), family=WGRAD_MFMA, G=21, n_pb=21)
    _is(_c(BWD_WEIGHT, 300, 8, 14, 14, 16), family=WGRAD_MFMA, G=512, n_pb=525)
    _is(_c(BWD_WEIGHT, 50, 9, 7, 7, 16), family=WGRAD_MFMA, grid_y=1)
    _is(_c(BWD_WEIGHT, 12, 24, 14, 14, 24), family=WGRAD_MFMA, grid_y=2)
    for co, co_ld in ((17, 32), (33, 64), (65, 128), (129, 192)):      # blocks of 32 / 32 / 64 / 64 channels
        _is(_c(BWD_WEIGHT, 12, 16, 14, 14, co), family=WGRAD_MFMA, reduce=R_SCATTER, co_ld=co_ld)
    _is(_c(BWD_WEIGHT, 15, 3, 24, 24, 23), family=WGRAD_VEC, slabs=15, reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 16, 2, 24, 24, 32), family=WGRAD_VEC, slabs=16, reduce=R_SLAB_SUM)
    _is(_c(BWD_WEIGHT, 16, 2, 24, 24, 32, acc=1, w_off=4), family=WGRAD_VEC, slabs=16, reduce=R_COLSUM_ACCUM)
    _is(_c(BWD_WEIGHT, 8, 8, 16, 16, 16), family=WGRAD_MFMA, G=16, reduce=R_SLAB_SUM)
    _is(_c(BWD_WEIGHT, 8, 8, 16, 16, 16, w_off=4), family=WGRAD_MFMA, G=16, reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 40, 1, 28, 28, 32), family=WGRAD_CONV1, slabs=40, reduce=R_SLAB_SUM)
    _is(_c(BWD_WEIGHT, 3, 4, 8, 8, 5), family=WGRAD_VEC, slabs=0, reduce=R_NONE)
    for op in (FWD, POOL2, BWD_INPUT):
        _is(_c(op, 3, 32, 14, 14, 64), family=MFMA)
        _is(_c(op, 3, 32, 14, 14, 64, img_mode=0), family=MFMA)
        _is(_c(op, 3, 32, 14, 14, 64, img_mode=1), family=IMG)
    for c in R.NAMED_CASES:
        assert c in R.CASES


def test_existing_conv_tests_reach_the_kernels_their_comments_claim():
    """tests/test_gpu_kernels.py: CONV_CASES ("matrix-core path", "widest matrix-core plane / VALU fallback") and test_conv3x3_bwd_full_mode
    ("the matrix-core weight-gradient kernel", "image slabs", "an image per workgroup", "a one-stage chain")"""
    for n, ci, h, w, co, pad in ((5, 8, 10, 12, 16, 1), (3, 13, 9, 11, 33, 0), (2, 16, 3, 40, 8, 1), (9, 24, 5, 5, 150, 1), (2, 40, 30, 30, 48, 0),
                                 (3, 8, 3, 3, 4, 0), (1, 64, 1, 1, 10, 1), (1, 8, 20, 120, 16, 1)):
        assert plan(FWD, n, ci, h, w, co, pad)["family"] in (MFMA, IMG), (n, ci, h, w, co, pad)
    _is(_c(FWD, 1, 8, 6, 130, 8), family=ROWS)
    for n, ci, h, w, co in ((12, 16, 14, 14, 24), (4, 40, 28, 28, 70), (50, 9, 7, 7, 16), (3, 32, 28, 28, 32)):
        _is(_c(BWD_WEIGHT, n, ci, h, w, co), family=WGRAD_MFMA)
    for n, ci, h, w, co in ((16, 1, 28, 28, 32), (11, 3, 30, 30, 5)):
        assert plan(BWD_WEIGHT, n, ci, h, w, co)["family"] == WGRAD_VEC and plan(BWD_WEIGHT, n, ci, h, w, co)["slabs"] > 1
    for n, ci, h, w, co in ((40, 1, 28, 28, 32), (33, 1, 32, 32, 16), (32, 1, 9, 7, 40)):
        _is(_c(BWD_WEIGHT, n, ci, h, w, co), family=WGRAD_CONV1)
    for n, ci, h, w, co in ((130, 32, 14, 14, 64), (129, 64, 7, 7, 128), (128, 32, 28, 28, 32), (131, 64, 14, 14, 64)):
        _is(_c(BWD_INPUT, n, ci, h, w, co), family=CHAIN, lin=1)


# ------------------------------------------------------------------------------------------------ the thresholds, from both sides
def test_threshold_ct_4_to_2_below_384_workgroup_slots():
    """conv3x3_mfma_plan: 128 output channels in blocks of 64 (CT 4) from 384 (image group, band, 64-channel block) slots, of 32 (CT 2) below:
    423 images of 7 x 7 in groups of 9 are 47 groups x 4 bands x 2 = 376; 424 are 48 x 4 x 2 = 384"""
    _is(_c(FWD, 423, 9, 7, 7, 128), family=MFMA, ct=2, grid_x=188, grid_y=4)
    _is(_c(FWD, 424, 9, 7, 7, 128), family=MFMA, ct=4, grid_x=192, grid_y=2)


def test_threshold_wh_2_below_768_workgroups():
    """eight waves a workgroup below 768 workgroups (no DMA staging: c_in = 9)"""
    _is(_c(FWD, 1719, 9, 7, 7, 32), family=MFMA, wh=2, dma=0, grid_x=764, grid_y=1)
    _is(_c(FWD, 1720, 9, 7, 7, 32), family=MFMA, wh=1, dma=0, grid_x=768, grid_y=1)
    _is(_c(FWD, 1720, 8, 7, 7, 32, img_mode=0), family=MFMA, wh=1, dma=1)      # DMA staging: four waves whatever the grid
    _is(_c(FWD, 9, 8, 7, 7, 32, img_mode=0), family=MFMA, wh=1, dma=1)


def test_threshold_tile_store_2_pow_19_outputs():
    _is(_c(FWD, 167, 8, 14, 14, 16), family=IMG, tile_store=0)      # 523 712 outputs
    _is(_c(FWD, 168, 8, 14, 14, 16), family=IMG, tile_store=1)      # 526 848
    _is(_c(POOL2, 168, 8, 14, 14, 16), family=IMG, tile_store=0)    # the pooled map never goes through the tile


def test_threshold_image_resident_kernel_one_unit_per_two_cus():
    """the default mode takes the image-resident kernel from 128 units (image groups x channel blocks)"""
    p = plan(FWD, 127, 8, 14, 14, 16, img_mode=1)
    assert p["family"] == IMG and p["img_t"] == 1
    _is(_c(FWD, 127, 8, 14, 14, 16), family=MFMA)
    _is(_c(FWD, 128, 8, 14, 14, 16), family=IMG)
    _is(_c(FWD, 128, 8, 14, 14, 16, img_mode=0), family=MFMA)
    _is(_c(BWD_INPUT, 128, 16, 14, 14, 8, acc=1), family=MFMA, acc=1)      # accumulate: never the image-resident kernel


def test_threshold_batch_128_chains_and_image_weight_gradient():
    """half the CU count: the one-stage chains and conv_wgrad_img_kernel from 128 images"""
    for op, ci, s, co in ((FWD, 32, 28, 32), (FWD, 32, 14, 64), (FWD, 64, 14, 64), (FWD, 64, 7, 128), (POOL2, 32, 28, 32), (POOL2, 32, 14, 64),
                          (POOL2, 64, 14, 64), (GAP, 64, 7, 128), (BWD_INPUT, 32, 14, 64), (BWD_INPUT, 64, 7, 128), (BWD_INPUT, 32, 28, 32),
                          (BWD_INPUT, 64, 14, 64)):
        assert plan(*_c(op, 127, ci, s, s, co))["family"] == IMG, (op, ci, s, co)
        for n in (128, 129, 257):
            _is(_c(op, n, ci, s, s, co), family=CHAIN, grid_x=min(n, 256), lin=int(op == BWD_INPUT))
        assert plan(*_c(op, 128, ci, s, s, co, img_mode=1))["family"] == IMG and plan(*_c(op, 128, ci, s, s, co, img_mode=0))["family"] in (MFMA, IMG)
    _is(_c(POOL2, 128, 64, 7, 7, 128), family=REFUSED)      # 7 x 7 has no whole 2 x 2 windows
    _is(_c(GAP, 128, 32, 14, 14, 64), family=IMG, gap=1)    # a gap the chain list does not hold
    _is(_c(FWD, 128, 64, 7, 7, 128, relu_bias=2), family=IMG)      # a bias without ReLU: neither the forward nor the LIN chain
    _is(_c(FWD, 128, 64, 7, 7, 128, layout=1), family=CHAIN, prep=1)      # prepped weights of 128 = 8 x 16 channels have the chain's pitch
    for ci, s, co in ((32, 14, 64), (64, 14, 64), (32, 28, 32)):
        _is(_c(BWD_WEIGHT, 127, ci, s, s, co), family=WGRAD_MFMA)
        for n in (128, 129):
            _is(_c(BWD_WEIGHT, n, ci, s, s, co), family=WGRAD_IMG, slabs=n, grid_x=n, reduce=R_SLAB_SUM)
    _is(_c(BWD_WEIGHT, 128, 64, 7, 7, 128), family=WGRAD_MFMA)      # left to the slab kernel


def test_threshold_weight_gradient_2048_pixels_and_image_slabs():
    _is(_c(BWD_WEIGHT, 42, 8, 7, 7, 16), family=WGRAD_MFMA)         # 2058 pixels
    _is(_c(BWD_WEIGHT, 41, 8, 7, 7, 16), family=WGRAD_VEC, slabs=0)  # 2009
    _is(_c(BWD_WEIGHT, 31, 1, 28, 28, 32), family=WGRAD_VEC)        # conv1_wgrad_kernel from 32 images
    _is(_c(BWD_WEIGHT, 32, 1, 28, 28, 32), family=WGRAD_CONV1)
    _is(_c(BWD_WEIGHT, 16, 3, 24, 24, 23), family=WGRAD_VEC, slabs=8)      # 9216 pixels, 69 channel pairs: 15 slabs asked, two images each
    _is(_c(BWD_WEIGHT, 14, 3, 24, 24, 23), family=WGRAD_VEC, slabs=0)      # 8064 pixels < 8192


# ------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("n,c_in,h,w,c_out,pad", [(2, 3, 5, 6, 4, 1), (2, 3, 5, 6, 4, 0), (1, 8, 4, 4, 5, 1), (3, 1, 7, 5, 2, 1), (2, 9, 3, 3, 17, 0)])
@pytest.mark.parametrize("layout", [0, 1])
def test_reference_equals_the_oracle_on_bits(n, c_in, h, w, c_out, pad, layout):
    """tests/conv_ref.py's numpy reference against the reference the project already trusts: O.Tensor.conv2d (layout 0), conv2d_direct_3x3
    (layout 1) and the mode = 1 backward of test_conv3x3_bwd_full_mode, on the integer data of the GPU tests"""
    from oracle import oracle as O
    case = _c(FWD, n, c_in, h, w, c_out, pad=pad, layout=layout)
    x, wt, bias, gy = R.operands(case)
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    xt, wtt, bt = O.Tensor(x), O.Tensor(wt), O.Tensor(bias)
    for b, bo in ((bias, bt), (None, None)):
        ref = xt.conv2d(wtt, bo, (1, 1), (pad, pad), (1, 1)) if layout == 0 else xt.conv2d_direct_3x3(wtt, bo, (1, 1), (pad, pad))
        np.testing.assert_array_equal(R.forward(x, wt, b, pad, layout, 0), ref.data()[:, :, :ho, :wo])
        np.testing.assert_array_equal(R.forward(x, wt, b, pad, layout, 1), ref.relu().data()[:, :, :ho, :wo])
    y = R.forward(x, wt, bias, pad, layout, 1)
    if ho % 2 == 0 and wo % 2 == 0:
        np.testing.assert_array_equal(R.pool2(y), O.Tensor(y).max_pool2d((2, 2), (2, 2), (0, 0)).data())
    mean, cnt = R.gap(y)
    np.testing.assert_array_equal(mean, (y.astype(np.float64).sum(axis=(2, 3)) / (ho * wo)).astype(np.float32))      # exact sums: one rounding
    assert (cnt == (y > 0).reshape(n, c_out, -1).sum(-1)).all()
    if pad != 1:
        return
    k = c_in * 9
    w_taper = wt if layout == 0 else np.ascontiguousarray(wt.reshape(c_out, k).T).reshape(c_out, c_in, 3, 3)
    O.Tape.reset()
    O.Tape.set_zero_sentinel(False)
    try:
        xg, wg = O.Tensor(x).requires_grad(), O.Tensor(w_taper).requires_grad()
        out = xg.conv2d(wg, None, (1, 1), (1, 1), (1, 1), mode=1)
        (out * O.Tensor(gy)).sum(None, False).backward()
        gx_ref = xg.grad()
        gw_ref = wg.grad() if layout == 0 else np.ascontiguousarray(wg.grad().reshape(k, c_out).T)
    finally:
        O.Tape.set_zero_sentinel(True)
        O.Tape.reset()
    np.testing.assert_array_equal(R.input_grad(gy, wt, c_in, layout), gx_ref)
    np.testing.assert_array_equal(R.weight_grad(x, gy, 1, layout), np.asarray(gw_ref).reshape(c_out, c_in, 3, 3))
