"""th_linear_fwd_ex's one-launch kernel takes its arguments in a form of its own (csrc/fwd_tick.hip: the operand pointers, the shape, the
tile rows, the grid width and a packed flag word up front, everything else in one struct behind them), and its tile waves ask for X and W
before they hold the bias and output pointers.  None of that may change a bit: H against th_linear_fwd, the carried slices' p / m / v
against th_adam_slices on copies, the counter one further.  The cases are what the argument path adds and tests/test_gpu_fwd_subtiles.py
does not reach: each flag bit alone, every instance by plan, a null bias / tick / slice list, the update guard, and one context launching
two shapes in a row (a packed word must not keep bits of the call before)."""
import ctypes as C

import numpy as np
import pytest

from taper_amd.hip import AdamFuse, AdamSlice

pytestmark = pytest.mark.gpu

T0 = 7
SLICE_SIZES = (1280, 10)      # more than one round of a 1 024-thread workgroup, and less than one wave


def fwd_plan(batch, inf, outf, subtiles=1):
    from taper_amd._lib import hip
    out = (C.c_int * 8)()
    assert hip.th_debug_linear_fwd_ex_plan(batch, inf, outf, subtiles, out) == 0, hip.th_last_error()
    return dict(zip(("one_launch", "rm", "rn", "waves", "cpw", "grid_x", "grid_y", "xcd"), out))


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.call("th_ctx_set_update_guard", None, None)
    c.call("th_linear_fwd_ex_set_subtiles", 1)
    c.close()


def _upload_off(ctx, a, off):
    """`a` on the device, `off` bytes past a 16-byte boundary (the pool's blocks are 16-byte aligned); -> (the block, the address)"""
    from taper_amd._lib import hip
    a = np.ascontiguousarray(a)
    buf = ctx.empty(a.size + 4)
    assert int(buf) % 16 == 0
    assert hip.th_memcpy_h2d(ctx.h, int(buf) + off, a.ctypes.data, a.nbytes) == 0
    return buf, int(buf) + off


def _floats(shape, seed):
    batch, inf, outf = shape
    rng = np.random.default_rng([seed, batch, inf, outf])
    return (rng.uniform(0, 1, (batch, inf)).astype(np.float32), rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32),
            rng.uniform(-0.1, 0.1, outf).astype(np.float32))


class Slices:
    """n carried slices twice over: side 0 for the forward launch, side 1 (copies, a counter of its own) for th_adam_slices"""

    def __init__(self, ctx, n, seed):
        rng = np.random.default_rng([seed, n])
        self.ctx, self.n = ctx, n
        self.dlr = ctx.upload(np.array([1e-3], np.float32))
        self.tick = [ctx.upload(np.array([T0, 0], np.int32)) for _ in range(2)]
        self.host = [[rng.uniform(-0.1, 0.1, k).astype(np.float32), (rng.standard_normal(k) * 1e-3).astype(np.float32),
                      rng.uniform(0, 1e-5, k).astype(np.float32), (rng.standard_normal(k) * 0.01).astype(np.float32)] for k in SLICE_SIZES[:n]]
        self.bufs, self.arr = [], []
        for side in range(2):
            arr, bufs = (AdamSlice * max(n, 1))(), []
            for i, h in enumerate(self.host):
                d = [ctx.upload(a) for a in h]
                bufs.append(d)
                arr[i] = AdamSlice(int(d[3]), h[0].size, AdamFuse(int(d[0]), int(d[1]), int(d[2]), int(self.tick[side]), int(self.dlr),
                                                                  0.9, 0.999, 1e-8, 1e-4))
            self.bufs.append(bufs)
            self.arr.append(arr)

    def state(self, side):
        return [[self.ctx.download(b, (h[0].size,)) for b in d[:3]] for d, h in zip(self.bufs[side], self.host)]

    def t(self, side):
        return int(self.ctx.download(self.tick[side], 2, np.int32)[0])

    def assert_untouched(self, side):
        for got, h in zip(self.state(side), self.host):
            for g, w in zip(got, h[:3]):
                assert g.tobytes() == w.tobytes()

    def assert_applied_like_th_adam_slices(self):
        if self.n:
            self.ctx.call("th_adam_slices", self.arr[1], self.n)
        for got, want, h in zip(self.state(0), self.state(1), self.host):
            for g, w, old in zip(got, want, h[:3]):
                assert g.tobytes() == w.tobytes()
                assert g.tobytes() != old.tobytes()       # ... and the update did happen


def _h_both_ways(ctx, shape, x_off=0, w_off=0, bias=True, relu=1, slices=None, n_slices=0, tick=None, seed=1):
    """H of th_linear_fwd_ex (carrying `slices` and `tick`) and of th_linear_fwd, on the same device operands"""
    batch, inf, outf = shape
    x, w, b = _floats(shape, seed)
    keep_x, dx = _upload_off(ctx, x, x_off)
    keep_w, dw = _upload_off(ctx, w, w_off)
    db = ctx.upload(b) if bias else None
    got, want = (ctx.upload(np.full(batch * outf, np.nan, np.float32)) for _ in range(2))
    ctx.call("th_linear_fwd_ex", dx, dw, db, got, batch, inf, outf, relu, slices, n_slices, tick)
    ctx.call("th_linear_fwd", dx, dw, db, want, batch, inf, outf, relu)
    got, want = ctx.download(got, (batch, outf)), ctx.download(want, (batch, outf))
    del keep_x, keep_w
    assert not np.isnan(got).any()
    assert got.tobytes() == want.tobytes(), f"{shape}: {np.count_nonzero(got != want)} of {got.size} elements differ from th_linear_fwd"
    return got


# (shape, X's and W's bytes off a 16-byte boundary): each vector-load flag alone and neither
@pytest.mark.parametrize("shape,x_off,w_off", [((18, 784, 20), 0, 4), ((5, 258, 10), 4, 4), ((18, 784, 20), 4, 4), ((18, 784, 20), 8, 12)],
                         ids=["w-off4", "5x258x10-both-off4", "18x784x20-both-off4", "x-off8-w-off12"])
def test_misaligned_operands(ctx, shape, x_off, w_off):
    assert fwd_plan(*shape)["one_launch"] == 1
    sl = Slices(ctx, 2, 11)
    _h_both_ways(ctx, shape, x_off, w_off, slices=sl.arr[0], n_slices=2, tick=sl.tick[0])
    sl.assert_applied_like_th_adam_slices()
    assert (sl.t(0), sl.t(1)) == (T0 + 1, T0)


# (shape, sub-tile rows, waves) as the plan must choose them
@pytest.mark.parametrize("shape,rm,waves", [((16, 64, 16), 16, 4), ((7, 20, 9), 16, 4), ((128, 784, 128), 16, 16), ((65, 256, 17), 16, 16),
                                            ((64, 784, 128), 8, 16)],
                         ids=["4w-16x64x16", "4w-7x20x9", "16w-128x784x128", "16w-65x256x17", "8x8-64x784x128"])
def test_every_instance_by_plan(ctx, shape, rm, waves):
    p = fwd_plan(*shape)
    assert (p["one_launch"], p["rm"], p["rn"], p["waves"]) == (1, rm, rm, waves), p
    assert p["grid_x"] == -(-shape[2] // rm) and p["grid_y"] == -(-shape[0] // rm) + 1, p
    sl = Slices(ctx, 2, 12)
    _h_both_ways(ctx, shape, slices=sl.arr[0], n_slices=2, tick=sl.tick[0])
    sl.assert_applied_like_th_adam_slices()
    assert (sl.t(0), sl.t(1)) == (T0 + 1, T0)


@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_bias_and_relu(ctx, bias, relu):
    shape = (7, 260, 9)
    h = _h_both_ways(ctx, shape, bias=bias, relu=relu)
    x, w, b = _floats(shape, 1)
    want = x.astype(np.float64) @ w.astype(np.float64).T + (b if bias else 0.0)
    if relu:
        want = np.maximum(want, 0.0)
    # 260 products of magnitude <= 0.1, summed in float32 in some order: |error| <= 260 * 2^-24 * sum |x w| <= 260 * 6e-8 * 26
    np.testing.assert_allclose(h, want, rtol=0, atol=260 * 2.0 ** -24 * 26)
    assert (h < 0).any() != bool(relu)


@pytest.mark.parametrize("with_tick", [False, True], ids=["notick", "tick"])
@pytest.mark.parametrize("n_extra", [0, 1, 2])
def test_slice_count_and_tick(ctx, n_extra, with_tick):
    sl = Slices(ctx, n_extra, 13)
    _h_both_ways(ctx, (7, 260, 9), slices=sl.arr[0] if n_extra else None, n_slices=n_extra, tick=sl.tick[0] if with_tick else None)
    sl.assert_applied_like_th_adam_slices()
    assert sl.t(0) == T0 + int(with_tick)           # (side 0's slices read this counter; nothing else may move it)
    assert sl.t(1) == T0
    if n_extra == 0 and not with_tick:
        # the spare row has nothing to do: a second word beside the counter and the rate are as uploaded
        assert ctx.download(sl.tick[0], 2, np.int32).tolist() == [T0, 0]
        assert ctx.download(sl.dlr, 1).tobytes() == np.array([1e-3], np.float32).tobytes()


def test_update_guard_holds_back_slices_and_tick(ctx):
    """the guard word non-zero: no slice, no tick, no step word -- and H as ever"""
    sl = Slices(ctx, 2, 14)
    words = ctx.upload(np.array([1, 41], np.uint32))
    try:
        ctx.call("th_ctx_set_update_guard", words, int(words) + 4)
        _h_both_ways(ctx, (7, 260, 9), slices=sl.arr[0], n_slices=2, tick=sl.tick[0])
        sl.assert_untouched(0)
        assert sl.t(0) == T0
        assert ctx.download(words, (2,), np.uint32).tolist() == [1, 41]
        # the word zero again: the same call applies them and advances both counters
        clear = ctx.upload(np.array([0, 41], np.uint32))
        ctx.call("th_ctx_set_update_guard", clear, int(clear) + 4)
        _h_both_ways(ctx, (7, 260, 9), slices=sl.arr[0], n_slices=2, tick=sl.tick[0])
        assert sl.t(0) == T0 + 1
        assert ctx.download(clear, (2,), np.uint32).tolist() == [0, 42]
    finally:
        ctx.call("th_ctx_set_update_guard", None, None)
    sl.assert_applied_like_th_adam_slices()


def test_two_shapes_on_one_context(ctx):
    """the flagship launch (XCD map, both vector flags, 8 x 8) and then a small ragged one with element loads, and back"""
    assert fwd_plan(64, 784, 128)["xcd"] == 1 and fwd_plan(7, 260, 9)["xcd"] == 0
    sl = Slices(ctx, 2, 15)
    _h_both_ways(ctx, (64, 784, 128), slices=sl.arr[0], n_slices=2, tick=sl.tick[0])
    assert sl.t(0) == T0 + 1
    _h_both_ways(ctx, (7, 260, 9), x_off=4, w_off=4)
    _h_both_ways(ctx, (7, 260, 9))
    _h_both_ways(ctx, (64, 784, 128), seed=2)
    assert sl.t(0) == T0 + 1
    sl.assert_applied_like_th_adam_slices()
