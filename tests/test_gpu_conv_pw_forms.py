"""Every kernel form of the exact pointwise convolution entry points (th_conv1x1_exact_fwd / _bwd_input / _bwd_weight, csrc/conv_pw.hip) against
an exact reference, compared on bits (np.array_equal on the uint32 view: the +0.0 of the input-gradient pixels no output reads included).

WHICH form a row of the case table takes is asserted, not assumed: tests/test_conv_pw_plan.py checks through th_debug_conv1x1_exact_plan (the
host function the entry points themselves launch from) that tests/conv_pw_ref.py's table reaches every form the plans can produce, and each
case here compares th_debug_last_conv_pw_config after the launch with what the plan predicted.  The operands are small integers
(tests/conv_pw_ref.py), so numpy's float64 result is exact and every summation order gives its float32 bits: there is no tolerance.  Beyond
the bits each case checks
  * unwritten outputs: without accumulate the output starts as NaN, and a hole stays one; with accumulate it starts from an integer y0, and
    after a stride-2 input gradient the pixels no output reads still hold y0's bits;
  * writes outside the output: y, gx and gw lie inside buffers whose margins (256 words either side) hold a bit pattern that must come back;
  * reads outside the operands: x, w, bias and gy lie inside NaN margins, and at stride 2 every pixel of x the convolution skips is NaN --
    the last partial tile, tiles that run over image boundaries, channel passes past c_in / c_out and channel tiles past the output must
    select or zero what lies outside;
  * the pool: its in-use figure is back where it was after each call (the partial slabs, the scatter temporary)."""
import ctypes as C

import numpy as np
import pytest

from tests import conv_pw_ref as R
from tests.conv_pw_ref import BWD_INPUT, BWD_WEIGHT, FWD
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
    out = (C.c_int * 9)()
    assert hip.th_debug_last_conv_pw_config(ctx.h, C.cast(out, C.c_void_p)) == 0
    return list(out)


def _call(ctx, name, *args):
    """the call, the pool's in-use figure unchanged by it; -> th_debug_last_conv_pw_config"""
    used = in_use(ctx)
    ctx.call(name, *args)
    assert in_use(ctx) == used, "the call kept workspace from the pool"
    return _last_config(ctx)


def _run(ctx, case):
    """-> the output's bits"""
    op, n, c_in, h, w, c_out, s, lay, rb, acc, off = case
    p = R.plan(*case)
    what = f"{R.form_name(R.form_of(*case))} {case} {p}"
    assert not p["refused"], what
    x, wt, bias, gy = R.operands(case)
    xp = R.poison_skipped(x, s)      # NaN in every pixel of x a stride-2 call must not load
    if op == FWD:
        relu, b = rb & 1, (bias if rb & 2 else None)
        bb, pb = operand(ctx, bias) if b is not None else (None, None)      # (bb: the allocation lives as long as the pointer is used)
        (bx, px), (bw, pw) = operand(ctx, xp), operand(ctx, wt, off)
        assert pw % 16 == off
        ref = R.forward(x, wt, b, s, lay, relu)
        out = Out(ctx, 1, ref.size, 0)
        cfg = _call(ctx, "th_conv1x1_exact_fwd", px, pw, pb, out.ptr, n, c_in, h, w, c_out, s, lay, relu)
    elif op == BWD_INPUT:
        (bg, pg), (bw, pw) = operand(ctx, gy), operand(ctx, wt, off)
        assert pw % 16 == off
        ref = R.input_grad(gy, wt, c_in, h, w, s, lay)
        y0 = R.initial(case, ref.shape) if acc else None
        out = Out(ctx, 1, ref.size, 0, None if y0 is None else y0.reshape(1, -1))
        cfg = _call(ctx, "th_conv1x1_exact_bwd_input", pg, pw, out.ptr, n, c_in, h, w, c_out, s, lay, acc)
        ref = ref if y0 is None else ref + y0
    else:
        (bx, px), (bg, pg) = operand(ctx, xp), operand(ctx, gy)
        ref = R.weight_grad(x, gy, s, lay)
        y0 = R.initial(case, ref.shape) if acc else None
        out = Out(ctx, 1, ref.size, off, None if y0 is None else y0.reshape(1, -1))
        assert out.ptr % 16 == off
        cfg = _call(ctx, "th_conv1x1_exact_bwd_weight", px, pg, out.ptr, n, c_in, h, w, c_out, s, lay, acc)
        ref = ref if y0 is None else ref + y0
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    body = out.check(ref.reshape(1, -1), what)
    bits = np.ascontiguousarray(body).view(np.uint32).copy()
    assert np.array_equal(bits, ref.reshape(1, -1).view(np.uint32)), what + ": the bits (a zero's sign)"
    if op == BWD_INPUT and acc and s == 2:      # the pixels no output reads were left alone: y0's bits, not y0 + 0.0
        mask = np.ones(ref.shape, bool)
        mask[:, :, ::2, ::2] = False
        assert np.array_equal(bits.reshape(ref.shape)[mask], y0.view(np.uint32)[mask]), what + ": an unread pixel was touched"
    assert cfg == R.predicted_config(p), what      # the query is what ran
    return bits


def _params(op):
    cs = [c for c in R.CASES if c[0] == op]
    return pytest.mark.parametrize("case", cs, ids=[R.case_id(c) for c in cs])


@_params(FWD)
def test_conv1x1_exact_fwd_exact(ctx, case):
    """y on bits: NaN going in, NaN around x / w / bias and in the skipped pixels of x, guard words around y, the pool restored, the launch
    the plan predicted"""
    _run(ctx, case)


@_params(BWD_INPUT)
def test_conv1x1_exact_bwd_input_exact(ctx, case):
    """gx on bits, every element written (the output starts as NaN; the unread pixels of stride 2 end as +0.0); with accumulate it starts from
    an integer y0 and ends as y0 + the gradient, the unread pixels untouched"""
    _run(ctx, case)


@_params(BWD_WEIGHT)
def test_conv1x1_exact_bwd_weight_exact(ctx, case):
    """gw on bits in the layout's memory order, through every reduce ending; gw 4 bytes off a 16-byte boundary where the case says so"""
    _run(ctx, case)


def test_accumulate_leaves_negative_zero_in_unread_pixels(ctx):
    """left untouched means untouched: -0.0 in an unread pixel of an accumulating stride-2 input gradient keeps its sign bit (y0 + 0.0 would
    lose it)"""
    case = R._c(BWD_INPUT, 2, 3, 5, 6, 4, 2, acc=1)
    op, n, c_in, h, w, c_out, s, lay, rb, acc, off = case
    x, wt, bias, gy = R.operands(case)
    y0 = np.full((n, c_in, h, w), -0.0, np.float32)
    (bg, pg), (bw, pw) = operand(ctx, gy), operand(ctx, wt)
    out = Out(ctx, 1, y0.size, 0, y0.reshape(1, -1))
    _call(ctx, "th_conv1x1_exact_bwd_input", pg, pw, out.ptr, n, c_in, h, w, c_out, s, lay, 1)
    ref = R.input_grad(gy, wt, c_in, h, w, s, lay) + y0
    ref[:, :, 1::2, :] = -0.0
    ref[:, :, :, 1::2] = -0.0
    body = out.check(ref.reshape(1, -1), "negative zeros")
    assert np.array_equal(np.ascontiguousarray(body).view(np.uint32), ref.reshape(1, -1).view(np.uint32))


@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("op", range(3), ids=R.OP_NAMES)
def test_two_runs_give_identical_bits(ctx, op, s):
    """no atomics anywhere: a second run of one case (several tiles, three images, a ragged channel tile) gives the first run's bits"""
    case = R._c(op, 3, 9, 33, 20, 17, s)
    np.testing.assert_array_equal(_run(ctx, case), _run(ctx, case))


GOOD = dict(n=2, c_in=3, h=5, w=6, c_out=4, s=2, lay=0, flag=0)
BAD_ARGS = [("n", 0, "bad geometry"), ("c_in", 0, "bad geometry"), ("h", 0, "bad geometry"), ("w", -1, "bad geometry"), ("c_out", 0, "bad geometry"),
            ("s", 0, "stride must be 1 or 2"), ("s", 3, "stride must be 1 or 2"), ("s", -2, "stride must be 1 or 2"),
            ("lay", 2, "weight_layout"), ("lay", -1, "weight_layout"), ("flag", 2, None), ("flag", -1, None)]


@pytest.mark.parametrize("op", range(3), ids=R.OP_NAMES)
def test_refusals_by_name_with_nothing_written(ctx, op):
    """null pointers, sizes below 1, a stride other than 1 or 2, layout or flag out of range: each refused with the function's name in the
    message, nothing taken from the pool, nothing launched (the output keeps its NaN), and a valid call afterwards still gives the right bits"""
    from taper_amd._lib import TaperError
    name = R.ENTRY_POINTS[op]
    case = R._c(op, 2, 3, 5, 6, 4, 2)
    x, wt, bias, gy = R.operands(case)
    (bx, px), (bw, pw), (bg, pg) = operand(ctx, x), operand(ctx, wt), operand(ctx, gy)
    out = Out(ctx, 1, (gy, x, wt)[op].size, 0)
    flag_word = "relu" if op == FWD else "accumulate"

    def args(ptrs, g):
        geo = (g["n"], g["c_in"], g["h"], g["w"], g["c_out"], g["s"], g["lay"], g["flag"])
        if op == FWD:
            return (ptrs[0], ptrs[1], None, ptrs[2]) + geo
        return tuple(ptrs) + geo

    ptrs = {FWD: (px, pw, out.ptr), BWD_INPUT: (pg, pw, out.ptr), BWD_WEIGHT: (px, pg, out.ptr)}[op]
    used = in_use(ctx)
    for i in range(3):
        bad = list(ptrs)
        bad[i] = None
        with pytest.raises(TaperError, match=f"{name}: null argument"):
            ctx.call(name, *args(bad, GOOD))
    for key, v, word in BAD_ARGS:
        with pytest.raises(TaperError, match=f"{name}: .*{word or flag_word}"):
            ctx.call(name, *args(ptrs, dict(GOOD, **{key: v})))
    assert in_use(ctx) == used, "a refused call kept workspace"
    ctx.sync()
    out.check(np.full((1, out.shape[1]), np.nan, np.float32), "the refused calls wrote nothing")
    _run(ctx, case)
