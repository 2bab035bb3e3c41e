"""Every kernel form of the 3x3 convolution entry points (th_conv3x3_fwd / _pool2_fwd / _gap_fwd / _bwd_input / _bwd_weight) against an exact
reference, compared on bits.

WHICH form a row of the case table takes is asserted, not assumed: tests/test_conv_plan.py checks through th_debug_conv3x3_plan (the host
function the entry points themselves launch from) that tests/conv_ref.py's table reaches every form the dispatch can produce, and each case
here compares th_debug_last_conv_config after the launch with what the plan predicted.  The operands are small integers (tests/conv_ref.py),
so numpy's float64 result is exact and every summation order gives its float32 bits: there is no tolerance.  Beyond the bits each case checks
  * unwritten outputs: without accumulate the output starts as NaN, and a hole stays one; with accumulate it starts from an integer y0;
  * writes outside the output: y, gx, gw, the pooled map and the gap pair lie inside buffers whose margins (256 words either side) hold a
    bit pattern that must come back;
  * reads outside the operands: x, w, bias and gy lie inside NaN margins -- halo taps, ragged last bands, the last partial image group,
    channel passes past c_in and channel tiles past c_out must select or zero what lies outside, never multiply it by zero;
  * the pool: its in-use figure is back where it was after each call (prepped weights, partial slabs, the scatter temporary)."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_ref as R
from tests.conv_ref import BWD_INPUT, BWD_WEIGHT, CHAIN, FWD, GAP, IMG, MFMA, POOL2, REFUSED
from tests.gpu_guard import Out, in_use, operand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _last_config(ctx):
    from taper_amd._lib import hip
    out = (C.c_int * 6)()
    assert hip.th_debug_last_conv_config(ctx.h, C.cast(out, C.c_void_p)) == 0
    return list(out)


def predicted_config(p):
    """what th_debug_last_conv_config reports after a launch of plan p (matrix-core families)"""
    if p["family"] == CHAIN:
        return [p["ct"], 8, 8, p["grid_x"], 1, p["pool"]]
    if p["family"] == IMG:
        return [p["ct"], 4 if p["wp"] else 2, p["tpw"], p["grid_x"], p["img_t"], p["pool"]]
    return [p["ct"], p["dma"], p["wh"], p["grid_x"], p["grid_y"], p["pool"]]


def _call(ctx, case, name, *args):
    """the call under the case's th_debug_set_conv_img mode, the pool's in-use figure unchanged by it; -> th_debug_last_conv_config"""
    im = case[11]
    used = in_use(ctx)
    try:
        if im != -1:
            ctx.call("th_debug_set_conv_img", im)
        ctx.call(name, *args)
        cfg = _last_config(ctx)
    finally:
        if im != -1:
            ctx.call("th_debug_set_conv_img", -1)
    assert in_use(ctx) == used, "the call kept workspace from the pool"
    return cfg


def _run(ctx, case):
    op, n, c_in, h, w, c_out, pad, lay, rb, acc, off, im = case
    p = R.plan(*case)
    what = f"{R.form_name(R.form_of(*case))} {case} {p}"
    assert p["family"] != REFUSED, what
    x, wt, bias, gy = R.operands(case)
    relu, b = rb & 1, (bias if rb & 2 else None)
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    bb, pb = operand(ctx, bias) if b is not None else (None, None)      # (bb: the allocation lives as long as the pointer is used)
    if op in (FWD, POOL2, GAP):
        (bx, px), (bw, pw) = operand(ctx, x), operand(ctx, wt, off)
        assert pw % 16 == off
        y = R.forward(x, wt, b, pad, lay, relu)
        if op == FWD:
            out = Out(ctx, 1, y.size, 0)
            cfg = _call(ctx, case, "th_conv3x3_fwd", px, pw, pb, out.ptr, n, c_in, h, w, c_out, pad, lay, relu)
            out.check(y.reshape(1, -1), what)
        elif op == POOL2:
            ref = R.pool2(y)
            out = Out(ctx, 1, ref.size, 0)
            cfg = _call(ctx, case, "th_conv3x3_pool2_fwd", px, pw, pb, out.ptr, n, c_in, h, w, c_out, pad, relu)
            out.check(ref.reshape(1, -1), what)
        else:
            mean, cnt = R.gap(y)
            om, oc = Out(ctx, 1, mean.size, 0), Out(ctx, 1, cnt.size, 0)
            cfg = _call(ctx, case, "th_conv3x3_gap_fwd", px, pw, pb, om.ptr, oc.ptr, n, c_in, h, w, c_out, pad, relu)
            om.check(mean.reshape(1, -1), what + " mean")
            oc.check(cnt.reshape(1, -1), what + " cnt")
    elif op == BWD_INPUT:
        (bg, pg), (bw, pw) = operand(ctx, gy), operand(ctx, wt)
        ref = R.input_grad(gy, wt, c_in, lay)
        y0 = R.initial(case, ref.shape) if acc else None
        out = Out(ctx, 1, ref.size, 0, None if y0 is None else y0.reshape(1, -1))
        cfg = _call(ctx, case, "th_conv3x3_bwd_input", pg, pw, out.ptr, n, c_in, h, w, c_out, pad, lay, acc)
        out.check((ref if y0 is None else ref + y0).reshape(1, -1), what)
    else:
        (bx, px), (bg, pg) = operand(ctx, x), operand(ctx, gy)
        ref = R.weight_grad(x, gy, pad, lay)
        y0 = R.initial(case, ref.shape) if acc else None
        out = Out(ctx, 1, ref.size, off, None if y0 is None else y0.reshape(1, -1))
        assert out.ptr % 16 == off
        cfg = _call(ctx, case, "th_conv3x3_bwd_weight", px, pg, out.ptr, n, c_in, h, w, c_out, pad, lay, acc)
        out.check((ref if y0 is None else ref + y0).reshape(1, -1), what)
        return
    if p["family"] in (MFMA, IMG, CHAIN):      # the query is what ran
        assert cfg == predicted_config(p), what


def _cases(op, refused=False):
    return [c for c in R.CASES if c[0] == op and (R.plan(*c)["family"] == REFUSED) == refused]


def _params(op):
    cs = _cases(op)
    return pytest.mark.parametrize("case", cs, ids=[R.case_id(c) for c in cs])


@_params(FWD)
def test_conv3x3_fwd_exact(ctx, case):
    """y on bits: NaN going in, NaN around x / w / bias, guard words around y, the pool restored, the launch the plan predicted"""
    _run(ctx, case)


@_params(POOL2)
def test_conv3x3_pool2_fwd_exact(ctx, case):
    """the pooled map of the ReLU output on bits (the full-resolution map is never written)"""
    _run(ctx, case)


@_params(GAP)
def test_conv3x3_gap_fwd_exact(ctx, case):
    """plane means and counts of positive outputs on bits.  The mean is the one value with a rounding -- an exact integer plane sum divided by
    the pixel count -- and the kernels divide (`sum / (float)pixels`, correctly rounded), which tests/conv_ref.py restates in float32: no ulp
    allowance was needed"""
    _run(ctx, case)


@_params(BWD_INPUT)
def test_conv3x3_bwd_input_exact(ctx, case):
    """gx on bits; with accumulate it starts from an integer y0 and ends as y0 + the gradient"""
    _run(ctx, case)


@_params(BWD_WEIGHT)
def test_conv3x3_bwd_weight_exact(ctx, case):
    """gw on bits in the layout's memory order, through every reduce ending; gw 4 bytes off a 16-byte boundary where the case says so"""
    _run(ctx, case)


REFUSED_CASES = [c for op in (FWD, BWD_INPUT) for c in _cases(op, refused=True)]


@pytest.mark.parametrize("case", REFUSED_CASES, ids=[R.case_id(c) for c in REFUSED_CASES])
def test_refused_shape_holds_no_workspace(ctx, case):
    """c_in = 3 on a 72 x 72 plane ((h + 2)(w + 2) x 32 B = 175 KB > 160 KB), and the same plane as an input gradient: the vector-ALU path
    refuses it by name, launches nothing, leaves the pool's in-use figure where it was, and a valid call afterwards still gives the right bits"""
    from taper_amd._lib import TaperError
    op, n, c_in, h, w, c_out, pad, lay, rb, acc, off, im = case
    x, wt, bias, gy = R.operands(case)
    (bx, px), (bw, pw), (bg, pg) = operand(ctx, x), operand(ctx, wt), operand(ctx, gy)
    out = Out(ctx, 1, (gy if op == FWD else x).size, 0)
    used = in_use(ctx)
    with pytest.raises(TaperError, match="72x72 plane does not fit the LDS tile"):
        if op == FWD:
            ctx.call("th_conv3x3_fwd", px, pw, None, out.ptr, n, c_in, h, w, c_out, pad, lay, 0)
        else:
            ctx.call("th_conv3x3_bwd_input", pg, pw, out.ptr, n, c_in, h, w, c_out, pad, lay, acc)
    assert in_use(ctx) == used, "the refused call kept its prepped weights"
    ctx.sync()
    out.check(np.full((1, out.shape[1]), np.nan, np.float32), "the refused call wrote nothing")
    _run(ctx, R._c(FWD, 2, 3, 9, 6, 7))
