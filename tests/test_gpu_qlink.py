"""Int8 links through the classifier on the GPU (csrc/qgemm_i8.hip's th_linear_q8q8_fwd_link, Module.quantize_static_linked):
the Linear product that writes the next layer's codes and sums its own rows, against the numpy restatement of tests/qlink_ref.py and
against the unlinked calls on the device; the linked twins against the unlinked twins.  Every comparison is on bits."""
import ctypes as C

import numpy as np
import pytest

from tests import qlink_ref as L
from tests import qstatic_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64                 # bytes (codes) or words (f32) on either side of a destination
GUARD_BYTE, FILL_BYTE = 0xA5, 0x5A
GUARD_BITS = 0xFFA5C3E1    # a NaN payload no computation produces
FN = "th_linear_q8q8_fwd_link"


def _lib():
    from taper_amd._lib import hip
    return hip


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _in_use(ctx):
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(ctx.h, C.byref(r), C.byref(u)) == 0
    return u.value


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _padded(codes, pitch, fill=0):
    rows, k = codes.shape
    out = np.full((rows, pitch), fill, np.int8)
    out[:, :k] = codes
    return out


def plan(B, K, N):
    out = (C.c_int * 4)()
    assert _lib().th_debug_q8q8_plan(B, K, N, C.cast(out, C.c_void_p)) == 0
    return dict(zip(("skinny", "tiles_m", "tiles_n", "grid"), out))


# ---------------------------------------------------------------- 1: the product with a destination
# (M, N, K): every M, N and K of the issue's sets, each N and K in both forms (32 x 32 tiles up to 256 rows, 128 x 128 above)
CASES = [(1, 1, 1), (1, 129, 784), (1, 16, 65), (31, 15, 17), (31, 128, 64), (33, 16, 65), (33, 33, 784), (33, 17, 1), (256, 17, 64), (256, 129, 65),
         (257, 128, 17), (257, 1, 784), (257, 33, 1), (257, 15, 64), (257, 16, 65), (300, 129, 65), (300, 17, 64), (300, 16, 1), (300, 33, 17), (300, 128, 784)]
PARAMS = [(1.0, (0.0, 1.0)), (0.0173, (-0.31, 0.0024))]      # (sx, {mw, sw}): pure integers (pins the lane maps), then a float codec
BPARAMS = (-0.27, 0.0019)
COMBOS = ((0, 0), (1, 0), (1, 1), (0, 1))                    # (bias, relu)


def test_case_table_covers_both_forms_and_ragged_tiles():
    assert {c[0] for c in CASES} == {1, 31, 33, 256, 257, 300}
    assert {c[1] for c in CASES} == {1, 15, 16, 17, 33, 128, 129}
    assert {c[2] for c in CASES} == {1, 17, 64, 65, 784}
    assert len(set(CASES)) == len(CASES)
    plans = {c: plan(c[0], c[2], c[1]) for c in CASES}
    for skinny, tile in ((1, 32), (0, 128)):
        mine = [c for c in CASES if plans[c]["skinny"] == skinny]
        assert {c[1] for c in mine} == {1, 15, 16, 17, 33, 128, 129} and {c[2] for c in mine} == {1, 17, 64, 65, 784}, skinny
        assert any(c[0] % tile for c in mine) and any(c[1] % tile for c in mine)                      # ragged in M and in N
        assert any(plans[c]["tiles_m"] > 1 for c in mine) and any(plans[c]["tiles_n"] > 1 for c in mine)      # more than one tile each way
        assert all(plans[c]["tiles_m"] == -(-c[0] // tile) and plans[c]["tiles_n"] == -(-c[1] // tile) for c in mine)
    assert plan(256, 64, 16)["skinny"] == 1 and plan(257, 64, 16)["skinny"] == 0                       # the switch at 256 rows


def _operands(M, N, K, seed):
    """int8 codes over the full range from two different generators (tests/test_gpu_qstatic.py's)"""
    rng = np.random.default_rng(seed)
    qx = rng.integers(-128, 128, (M, K)).astype(np.int8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    qw = ((n * 37 + k * 101 + (n * k) % 7 + rng.integers(0, 3, (N, K))) % 256 - 128).astype(np.int8)
    for q in (qx, qw):
        if q.size >= 2:
            q.reshape(-1)[0], q.reshape(-1)[-1] = -128, 127
    return qx, qw, rng.integers(-128, 128, N).astype(np.int8)


def _pc_pairs(wp, N):
    """a pair per row that differs from row to row"""
    n = np.arange(N)
    return np.stack([f32(wp[0]) + f32(0.125) * (n % 5).astype(f32), f32(wp[1]) * (1 + n % 3).astype(f32)], axis=1).astype(f32)


class Layer:
    """the operands of one product on the device: x padded with zeros, W's padding filled with a non-zero code (it must not matter)"""

    def __init__(self, ctx, qx, qw, qb, pitch_x=None, pitch_w=None):
        (self.M, self.K), self.N = qx.shape, qw.shape[0]
        self.ctx, self.qx, self.qw, self.qb = ctx, qx, qw, qb
        self.pitch_x, self.pitch_w = pitch_x or L.up16(self.K), pitch_w or -(-self.K // 64) * 64
        self.dx, self.dw = ctx.upload(_padded(qx, self.pitch_x).view(np.uint8)), ctx.upload(_padded(qw, self.pitch_w, 0x55).view(np.uint8))
        self.drs = ctx.upload(L.row_sums(qx))
        self.db, self.dbp = ctx.upload(qb.view(np.uint8)), ctx.upload(np.array(BPARAMS, f32))

    def args(self, sx, wparams, bias, relu, own):
        pc = int(np.ndim(wparams) == 2)
        self.keep = (self.ctx.upload(np.array([sx], f32)), self.ctx.upload(np.asarray(wparams, f32)))
        return (self.dx, self.pitch_x, None if own else self.drs, self.keep[0], self.M, self.K, self.dw, self.pitch_w, self.N, self.keep[1], pc,
                self.db if bias else None, self.dbp if bias else None, relu)

    def codes(self, sx, wparams, bias, relu, sy, pitch_y, own=False):
        """one call with a codes destination, pre-filled and between guard bytes -> every byte of the rows [M, pitch_y]"""
        ctx, M = self.ctx, self.M
        dsy = ctx.upload(np.array([sy], f32))
        buf = np.full(2 * GUARD + M * pitch_y, GUARD_BYTE, np.uint8)
        buf[GUARD:GUARD + M * pitch_y] = FILL_BYTE
        dq = ctx.upload(buf)
        args = self.args(sx, wparams, bias, relu, own)
        before = _in_use(ctx)
        ctx.call(FN, *args, None, dsy, dq.offset(GUARD), pitch_y)
        assert _in_use(ctx) == before                    # the call allocates nothing
        out = ctx.download(dq, buf.shape, np.uint8)
        assert (out[:GUARD] == GUARD_BYTE).all() and (out[GUARD + M * pitch_y:] == GUARD_BYTE).all(), "bytes around the codes were written"
        return out[GUARD:GUARD + M * pitch_y].view(np.int8).reshape(M, pitch_y)

    def f32(self, sx, wparams, bias, relu, own=False):
        """one call with the f32 destination, NaN-filled between guard words"""
        ctx, n = self.ctx, self.M * self.N
        ybuf = ctx.upload(np.full(n + 2 * GUARD, GUARD_BITS, np.uint32))
        ctx.call("th_fill_f32", ybuf.offset(4 * GUARD), float("nan"), n)
        ctx.call(FN, *self.args(sx, wparams, bias, relu, own), ybuf.offset(4 * GUARD), None, None, 0)
        out = ctx.download(ybuf, (n + 2 * GUARD,), np.uint32)
        assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + n:] == GUARD_BITS).all(), "words around the output were written"
        return out[GUARD:GUARD + n].view(f32).reshape(self.M, self.N)

    def unlinked_codes(self, sx, wparams, bias, relu, sy, pitch_y):
        """th_quantize_act_int8 of th_linear_q8q8_fwd's (or _pc's) output, on the device"""
        ctx, M, N = self.ctx, self.M, self.N
        a = self.args(sx, wparams, bias, relu, False)
        y, dsy = ctx.empty(M * N), ctx.upload(np.array([sy], f32))
        ctx.call("th_linear_q8q8_fwd_pc" if a[10] else "th_linear_q8q8_fwd", *a[:10], *a[11:], y)
        dq, drs = ctx.upload(np.full(M * pitch_y, FILL_BYTE, np.uint8)), ctx.empty(M, np.int32)
        ctx.call("th_quantize_act_int8", y, M, N, dsy, dq, pitch_y, drs)
        return ctx.download(dq, (M, pitch_y), np.int8)


def _ref(lay, sx, wp, bias, relu):
    return L.linear_f32(lay.qx, sx, lay.qw, wp, lay.qb if bias else None, BPARAMS, relu)


def _scale_for(ref):
    """the next layer's scale: the outer 40 % of the range saturates (a finite positive scale whatever the values)"""
    top = f32(np.abs(ref[np.isfinite(ref)]).max(initial=0))
    return f32(top * f32(0.6) / f32(127)) if top > 0 else f32(1)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_codes_destination_is_the_codec_of_the_f32_product(ctx, case):
    M, N, K = case
    qx, qw, qb = _operands(M, N, K, seed=M * 7919 + N * 31 + K)
    lay = Layer(ctx, qx, qw, qb, pitch_x=L.up16(K) + 16 * (CASES.index(case) % 3))
    for pc in (0, 1):
        for (sx, wp), (bias, relu) in zip(PARAMS + PARAMS, COMBOS):
            wparams = _pc_pairs(wp, N) if pc else wp
            sy = _scale_for(_ref(lay, sx, wparams, bias, relu))
            for pitch_y in (L.up16(N), L.up16(N) + 64):
                what = str((case, "pc", pc, sx, "bias", bias, "relu", relu, "pitch_y", pitch_y))
                ref = L.linear_q8q8_codes(qx, sx, qw, wparams, qb if bias else None, BPARAMS, relu, sy, pitch_y)
                got = lay.codes(sx, wparams, bias, relu, sy, pitch_y)
                assert (got[:, N:] == 0).all(), "padding bytes: " + what
                np.testing.assert_array_equal(got.view(np.uint8), ref.view(np.uint8), err_msg=what)
                np.testing.assert_array_equal(got.view(np.uint8), lay.unlinked_codes(sx, wparams, bias, relu, sy, pitch_y).view(np.uint8), err_msg=what)
    if N > 1 and K > 16:
        assert len(np.unique(got[:, :N])) > 8 and np.abs(got.astype(int)).max() >= 127      # the codes spread and saturate


@pytest.mark.parametrize("M,N,pitch_y", [(257, 128, 192), (5, 32, 64)], ids=["128x128-form", "few-rows-form"])
def test_padding_beyond_the_last_column_tile_is_written(ctx, M, N, pitch_y):
    """N fills its column tiles exactly: the bytes N .. pitch_y - 1 lie in no tile, and are written 0 all the same"""
    qx, qw, qb = _operands(M, N, 65, seed=M)
    lay = Layer(ctx, qx, qw, qb)
    assert N % (32 if plan(M, 65, N)["skinny"] else 128) == 0
    for own in (False, True):
        for pc in (0, 1):
            sx, wp = PARAMS[1]
            wparams = _pc_pairs(wp, N) if pc else wp
            sy = _scale_for(_ref(lay, sx, wparams, 1, 0))
            got = lay.codes(sx, wparams, 1, 0, sy, pitch_y, own)
            assert (got[:, N:] == 0).all()
            np.testing.assert_array_equal(got, L.linear_q8q8_codes(qx, sx, qw, wparams, qb, BPARAMS, 0, sy, pitch_y))


def test_codec_edges_on_integer_data(ctx):
    """sx = sw = 1, mw = 0: the value is the integer t itself.  A scale of 2 puts every odd t on a .5 tie (rounded away from zero), both
    ends saturate; a NaN scale-in gives the code 0, an infinite one saturates by sign (0 * inf: NaN, the code 0)"""
    rng = np.random.default_rng(5)
    M, N, K = 40, 48, 24
    qx = rng.integers(-20, 21, (M, K)).astype(np.int8)
    qw = rng.integers(-128, -120, (N, K)).astype(np.int8)      # decoded weights 0 .. 7: |t| stays within a few thousand, exact in f32
    qx[0], qx[1], qx[2] = 0, 20, -20                            # t = 0 everywhere; far above 254; far below -256
    lay = Layer(ctx, qx, qw, np.zeros(N, np.int8))
    t = L.linear_f32(qx, 1.0, qw, (0.0, 1.0))
    assert (t == np.round(t)).all() and (np.abs(t) % 2 == 1).any() and t.max() > 256 > -256 > t.min() and (t == 0).any()
    for sx, sy in ((1.0, 2.0), (1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (float("-inf"), 1.0), (1.0, float("inf")), (1.0, float("nan"))):
        ref = L.linear_q8q8_codes(qx, sx, qw, (0.0, 1.0), None, None, False, sy, N)
        np.testing.assert_array_equal(lay.codes(sx, (0.0, 1.0), 0, 0, sy, N), ref, err_msg=str((sx, sy)))
        if sx == 1.0 and sy == 2.0:
            odd = np.abs(t) % 2 == 1
            inside = odd & (np.abs(t) < 250)
            np.testing.assert_array_equal(ref[:, :N][inside], (np.sign(t) * (np.abs(t) + 1) / 2)[inside].astype(np.int8))      # ties go away from zero
            assert ref.max() == 127 and ref.min() == -128
        if np.isinf(sx):
            assert set(np.unique(ref)) == {-128, 0, 127}
        if np.isnan(sx) or np.isnan(sy):
            assert (ref == 0).all()


# ---------------------------------------------------------------- 2: the product sums its own rows
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_own_row_sums_give_the_bits_of_the_explicit_sums(ctx, case):
    M, N, K = case
    qx, qw, qb = _operands(M, N, K, seed=M * 7919 + N * 31 + K + 1)
    lay = Layer(ctx, qx, qw, qb, pitch_x=L.up16(K) + 16 * (CASES.index(case) % 3))
    for pc in (0, 1):
        for (sx, wp), (bias, relu) in zip(PARAMS, ((1, 0), (0, 1))):
            wparams = _pc_pairs(wp, N) if pc else wp
            ref = _ref(lay, sx, wparams, bias, relu)
            what = str((case, "pc", pc, sx))
            np.testing.assert_array_equal(_bits(lay.f32(sx, wparams, bias, relu, own=False)), _bits(ref), err_msg=what)      # the link call IS the product
            np.testing.assert_array_equal(_bits(lay.f32(sx, wparams, bias, relu, own=True)), _bits(ref), err_msg=what)
            sy, pitch_y = _scale_for(ref), L.up16(N) + 16
            np.testing.assert_array_equal(lay.codes(sx, wparams, bias, relu, sy, pitch_y, own=True), lay.codes(sx, wparams, bias, relu, sy, pitch_y, own=False),
                                          err_msg=what)


@pytest.mark.parametrize("M", [3, 300])
def test_own_row_sums_stop_at_the_last_piece_of_k(ctx, M):
    """K = 10 in rows of 64 bytes: the bytes 10 .. 15 are zero by contract, the pieces behind the first are never read as codes"""
    qx, qw, qb = _operands(M, 20, 10, seed=M)
    rows = _padded(qx, 64)
    rows[:, 16:] = 0x33                                         # beyond ceil(K / 16) pieces: must count as zero
    lay = Layer(ctx, qx, qw, qb, pitch_x=64)
    lay.dx = ctx.upload(rows.view(np.uint8))
    for sx, wp in PARAMS:
        np.testing.assert_array_equal(_bits(lay.f32(sx, wp, 1, 0, own=True)), _bits(_ref(lay, sx, wp, 1, 0)))


def test_own_row_sums_at_the_bound_of_the_sums(ctx):
    K = R.MAX_K
    qx, qw = np.full((1, K), -128, np.int8), np.full((1, K), 127, np.int8)
    lay = Layer(ctx, qx, qw, np.zeros(1, np.int8), pitch_x=K, pitch_w=K)
    t, rs = R.int_terms(qx, qw)
    assert rs[0] == -128 * K and t[0, 0] == -128 * 255 * K      # the largest |rs| and |t| there are: inside int32
    np.testing.assert_array_equal(lay.f32(1.0, (0.0, 1.0), 0, 0, own=True), t.astype(f32))
    for sx, wp in PARAMS:
        np.testing.assert_array_equal(_bits(lay.f32(sx, wp, 0, 0, own=True)), _bits(R.linear_q8q8(qx, sx, qw, wp)))


# ---------------------------------------------------------------- 3: refusals
def test_refusals_name_the_call_and_write_nothing(ctx):
    lib = _lib()
    M, N, K = 5, 20, 30
    qx, qw, qb = _operands(M, N, K, seed=9)
    lay = Layer(ctx, qx, qw, qb)
    sx, wp = PARAMS[1]
    pitch_y = 32
    dsy = ctx.upload(np.array([0.05], f32))
    dq = ctx.upload(np.full(2 * GUARD + M * pitch_y + 16, FILL_BYTE, np.uint8))
    dy = ctx.upload(np.full(M * N + 2 * GUARD, GUARD_BITS, np.uint32))
    base = lay.args(sx, wp, 1, 0, False)
    q, y = dq.offset(GUARD), dy.offset(4 * GUARD)

    def call(args=base, dest=(None, dsy, q, pitch_y)):
        conv = [int(a) if hasattr(a, "ptr") else a for a in (*args, *dest)]
        return getattr(lib, FN)(ctx.h, *conv)

    def with_(**kw):
        names = ("d_qx", "pitch_x", "d_rowsum", "d_xscale", "batch", "in_features", "d_qw", "pitch_w", "out_features", "d_wparams", "per_channel", "d_qb",
                 "d_bparams", "relu")
        a = dict(zip(names, base))
        a.update(kw)
        return tuple(a[n] for n in names)

    refused = [
        ("null argument", lambda: call(with_(d_qx=None))),
        ("null argument", lambda: call(with_(d_xscale=None))),
        ("null argument", lambda: call(with_(d_qw=None))),
        ("null argument", lambda: call(with_(d_wparams=None))),
        ("null argument", lambda: call(with_(d_bparams=None))),
        ("exactly one destination", lambda: call(dest=(None, dsy, None, pitch_y))),
        ("exactly one destination", lambda: call(dest=(y, dsy, q, pitch_y))),
        ("a codes destination needs d_yscale", lambda: call(dest=(None, None, q, pitch_y))),
        ("bad shape", lambda: call(with_(batch=-1))),
        ("bad shape", lambda: call(with_(in_features=0))),
        ("bad shape", lambda: call(with_(out_features=0))),
        ("in_features 65537 is above 65536", lambda: call(with_(in_features=65537, pitch_x=65552, pitch_w=65552))),
        ("the code pointers must be 16-byte aligned", lambda: call(with_(d_qx=lay.dx.offset(8)))),
        ("pitches 24 / 64", lambda: call(with_(pitch_x=24))),
        ("pitches 32 / 16", lambda: call(with_(pitch_w=16))),
        ("the codes destination must be 16-byte aligned", lambda: call(dest=(None, dsy, dq.offset(GUARD + 8), pitch_y))),
        ("pitch_y 24 must be a multiple of 16 and at least out_features 20", lambda: call(dest=(None, dsy, q, 24))),
        ("pitch_y 16 must be a multiple of 16 and at least out_features 20", lambda: call(dest=(None, dsy, q, 16))),
    ]
    before = _in_use(ctx)
    for want, refuse in refused:
        assert refuse() != 0, want
        msg = lib.th_last_error().decode()
        assert msg.startswith(FN + ": ") and want in msg, (want, msg)
    assert _in_use(ctx) == before
    assert call(with_(batch=0)) == 0                                    # an empty batch is a shape: nothing is launched
    assert call(with_(batch=0), dest=(y, None, None, 0)) == 0
    ctx.sync()
    assert (ctx.download(dy, (M * N + 2 * GUARD,), np.uint32) == GUARD_BITS).all(), "a refused call wrote"
    assert (ctx.download(dq, (2 * GUARD + M * pitch_y + 16,), np.uint8) == FILL_BYTE).all(), "a refused call wrote"
    # and the next valid calls succeed: codes with the sums given, f32 without
    np.testing.assert_array_equal(lay.codes(sx, wp, 1, 0, 0.05, pitch_y), L.linear_q8q8_codes(qx, sx, qw, wp, qb, BPARAMS, 0, 0.05, pitch_y))
    np.testing.assert_array_equal(_bits(lay.f32(sx, wp, 1, 0, own=True)), _bits(_ref(lay, sx, wp, 1, 0)))


# ---------------------------------------------------------------- 4: linked twins are the unlinked twins, bit for bit
CONVS, CHAIN, PER_CHANNEL, LINKS = 1, 2, 4, 16


def _pool_in_use():
    import taper_amd as T
    from taper_amd import hip
    return _in_use(hip.Ctx(handle=T.Device.ctx_handle()))


def _twin(model, calib, flags):
    from taper_amd._lib import host
    return model._quantize_static(host.tp_module_quantize_static_ex, "quantize_static_ex", calib, flags)


def _randomize(model, rng, scale=0.4):
    for p in model.parameters():
        p.set_data((scale * rng.standard_normal(p.numel())).astype(f32))
    return model


def _assert_same_tensors(a, b):
    np.testing.assert_array_equal(_bits(a.act_scales()), _bits(b.act_scales()))
    ta, tb = a.tensors(), b.tensors()
    assert len(ta) == len(tb)
    for (k1, c1, p1), (k2, c2, p2) in zip(ta, tb):
        assert k1 == k2
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))


def _linked_and_plain(model, calib, flags, links):
    """the twin with LINKS and the twin with the same flags without: the same scales and tensors, `links` boundaries in int8"""
    import taper_amd as T
    T.Tape.reset()
    linked, plain = _twin(model, calib, flags | LINKS), _twin(model, calib, flags)
    assert T.Tape.len() == 0
    assert linked.chain_links() == links, linked.chain_links()
    _assert_same_tensors(linked, plain)
    return linked, plain


def _assert_same_forward(linked, plain, x, shape):
    import taper_amd as T
    before = _pool_in_use()
    y = linked(T.Tensor(x, shape).requires_grad())
    assert T.Tape.len() == 0 and y.tape_node() == 0
    got = y.data()
    del y
    assert _pool_in_use() == before                      # every buffer of codes went back to the pool
    ref = plain(T.Tensor(x, shape)).data()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    return got


def _linear_ref(ts, scales, x, relus):
    """the restatement through a stack of Linears from the twin's tensors() and act_scales(): every boundary through the codec"""
    h = x
    for i, relu in enumerate(relus):
        (_, w, wp), (_, b, bp) = ts[2 * i], ts[2 * i + 1]
        h = L.linear_f32(R.quantize_act(h, scales[i])[0], scales[i], w.reshape(b.size, -1), np.asarray(wp, f32) if np.ndim(wp) == 2 else wp, b, bp, relu)
    return h


@pytest.mark.parametrize("per_channel", [0, 1], ids=["per-tensor", "per-channel"])
def test_linked_mlp_is_the_unlinked_mlp_bit_for_bit(per_channel):
    import taper_amd as T
    rng = np.random.default_rng(70 + per_channel)
    model = _randomize(T.Sequential([T.Linear(20, 33, True), T.ReLU(), T.Linear(33, 17, True), T.ReLU(), T.Linear(17, 10, True)]), rng)
    calib = [T.Tensor(rng.standard_normal((16, 20)).astype(f32), (16, 20)) for _ in range(2)]
    for flags in ((PER_CHANNEL if per_channel else 0), CONVS | CHAIN | (PER_CHANNEL if per_channel else 0)):
        linked, plain = _linked_and_plain(model, calib, flags, links=2)
        assert plain.chain_links() == 0 and linked.storage_bytes() == plain.storage_bytes()
        for B in (1, 5, 300):
            x = (1.5 * rng.standard_normal((B, 20))).astype(f32)      # beyond the calibration range here and there: codes saturate
            got = _assert_same_forward(linked, plain, x, (B, 20))
            np.testing.assert_array_equal(_bits(got), _bits(_linear_ref(linked.tensors(), linked.act_scales(), x, (True, True, False))))
    named = model.quantize_static_linked(calib, per_channel=bool(per_channel))
    assert named.chain_links() == 2
    np.testing.assert_array_equal(_bits(named(T.Tensor(x, (300, 20))).data()), _bits(got))


def _c3(T, ci, co, relu=True, **kw):
    return (T.Conv2dReLU if relu else T.Conv2d)(ci, co, (3, 3), None, (1, 1), **kw)


def _cnn(T, bn=False):
    front = [_c3(T, 1, 6), T.MaxPool2d((2, 2)), _c3(T, 6, 6, relu=not bn)] + ([T.BatchNorm2d(6), T.ReLU()] if bn else [])
    return T.Sequential(front + [T.MaxPool2d((2, 2)), T.Flatten(1), T.Linear(24, 12, True), T.ReLU(), T.Linear(12, 10, True)])


def _cnn_ref(ts, scales, x, pc):
    """the restatement of the CNN in the linked formulation: the second conv's pooled codes channel-last, the first Linear's rows re-laid"""
    from tests import qchain_ref as QC
    from tests import qconv_ref as Q
    from tests import qperchan_ref as P
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2), (_, w3, p3), (_, b3, q3), (_, w4, p4), (_, b4, q4) = ts
    conv = P.conv_q8q8_pc if pc else Q.conv_q8q8
    h = conv(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 6, 1, (3, 3)), p1, b1, q1, pad=(1, 1), relu=True)
    h = conv(Q.quantize_act_nchw(Q.max_pool(h, (2, 2), (2, 2)), scales[1])[0], scales[1], Q.taper_weight(w2, 6, 6, (3, 3)), p2, b2, q2, pad=(1, 1), relu=True)
    codes, _ = QC.max_pool_codes(Q.nhwc(Q.quantize_act_nchw(h, scales[2])[0], 16), 6, (2, 2), (2, 2))      # the pool on the Linear's codes
    rows = codes.reshape(x.shape[0], 4 * 16)
    flat = R.quantize_act(Q.max_pool(h, (2, 2), (2, 2)).reshape(x.shape[0], -1), scales[2])[0]               # the unlinked path's codes
    np.testing.assert_array_equal(rows, L.flatten_nhwc(flat.reshape(-1, 6, 2, 2), 16))
    h = L.linear_f32(rows, scales[2], L.relay_flatten(w3.reshape(12, 24), 6, 4, 16), p3, b3, q3, True)
    return L.linear_f32(R.quantize_act(h, scales[3])[0], scales[3], w4.reshape(10, 12), p4, b4, q4, False)


@pytest.mark.parametrize("per_channel", [0, 1], ids=["per-tensor", "per-channel"])
def test_linked_cnn_is_the_unlinked_cnn_bit_for_bit(per_channel):
    import taper_amd as T
    rng = np.random.default_rng(72 + per_channel)
    model = _randomize(_cnn(T), rng)
    shape = (4, 1, 8, 8)
    calib = [T.Tensor(rng.standard_normal(shape).astype(f32), shape) for _ in range(2)]
    flags = CONVS | CHAIN | (PER_CHANNEL if per_channel else 0)
    linked, plain = _linked_and_plain(model, calib, flags, links=3)
    assert plain.chain_links() == 1
    # the first Linear holds 12 rows of 2 x 2 pixels x 16 channel bytes instead of 12 rows of 24 codes padded to 64
    assert linked.storage_bytes() == plain.storage_bytes() - 12 * 64 + 12 * 4 * 16
    for B in (1, 3):
        x = (1.5 * rng.standard_normal((B, 1, 8, 8))).astype(f32)
        got = _assert_same_forward(linked, plain, x, (B, 1, 8, 8))
        ts = [(k, c, np.asarray(p, f32) if np.ndim(p) == 2 else p) for k, c, p in linked.tensors()]
        np.testing.assert_array_equal(_bits(got), _bits(_cnn_ref(ts, linked.act_scales(), x, per_channel)))
    named = model.quantize_static_linked(calib, per_channel=bool(per_channel))
    assert named.chain_links() == 3
    np.testing.assert_array_equal(_bits(named(T.Tensor(x, (3, 1, 8, 8))).data()), _bits(got))


def test_linked_cnn_with_a_batchnorm_folded_ahead_of_the_flatten_link():
    import taper_amd as T
    rng = np.random.default_rng(74)
    model = _cnn(T, bn=True)
    for p in model.parameters():
        p.set_data((0.4 * rng.standard_normal(p.numel()) + (1.0 if p.numel() == 6 else 0.0)).astype(f32))
    for b, v in zip(model.buffers(), (0.1 * rng.standard_normal(6), rng.uniform(0.5, 1.5, 6))):
        b.set_data(v.astype(f32))
    shape = (3, 1, 8, 8)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    linked, plain = _linked_and_plain(model, calib, CONVS | CHAIN, links=3)
    assert len(linked.affines()) == 1
    for B in (1, 3):
        _assert_same_forward(linked, plain, rng.standard_normal((B, 1, 8, 8)).astype(f32), (B, 1, 8, 8))


def test_linked_cnn_from_qat_layers():
    import taper_amd as T
    rng = np.random.default_rng(75)
    shape = (3, 1, 8, 8)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    plain = T.Sequential([_c3(T, 1, 6, seed=3), T.MaxPool2d((2, 2)), _c3(T, 6, 6, seed=5), T.MaxPool2d((2, 2)), T.Flatten(1), T.Linear(24, 12, True, seed=4), T.ReLU(),
                          T.Linear(12, 10, True, seed=6)])
    qat = T.Sequential([T.QATConv2d(1, 6, (3, 3), None, (1, 1), relu=True, seed=3), T.MaxPool2d((2, 2)), T.QATConv2d(6, 6, (3, 3), None, (1, 1), relu=True, seed=5),
                        T.MaxPool2d((2, 2)), T.Flatten(1), T.QATLinear(24, 12, True, seed=4), T.ReLU(), T.QATLinear(12, 10, True, seed=6)])
    for a, b in zip(plain.parameters(), qat.parameters()):
        np.testing.assert_array_equal(_bits(a.data()), _bits(b.data()))
    ref = plain.quantize_static_chain(calib)
    T.qat.enable()
    try:
        q = qat.quantize_static_linked(calib)
    finally:
        T.qat.disable()
    assert q.chain_links() == 3 and ref.chain_links() == 1
    _assert_same_tensors(q, ref)
    _assert_same_forward(q, ref, rng.standard_normal(shape).astype(f32), shape)


def test_a_captured_forward_replays_the_same_bits():
    import taper_amd as T
    from taper_amd import hip
    rng = np.random.default_rng(76)
    model = _randomize(_cnn(T), rng)
    shape = (3, 1, 8, 8)
    q = model.quantize_static_linked(T.Tensor(rng.standard_normal(shape).astype(f32), shape))
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    eager = q(x).data()
    c = hip.Ctx(handle=T.Device.ctx_handle())
    c.graph_begin()
    try:
        y = q(x)                                         # no allocation outside the pool, no synchronisation, no read-back
    finally:
        g = c.graph_end()
    try:
        for _ in range(2):
            c.graph_launch(g)
            T.Device.sync()
            np.testing.assert_array_equal(_bits(y.data()), _bits(eager))
    finally:
        del y
        c.graph_destroy(g)


# (what, layers, input shape, flags without LINKS, links with LINKS, links without)
def _lin_tail(T, k):
    return [T.Linear(k, 12, True), T.ReLU(), T.Linear(12, 10, True)]


NO_LINKS = [
    ("a sigmoid between two Linears", lambda T: [T.Linear(20, 12, True), T.Sigmoid(), T.Linear(12, 10, True)], (3, 20), CONVS | CHAIN, 0, 0),
    ("a Linear inside a nested Sequential", lambda T: [T.Linear(20, 12, True), T.ReLU(), T.Sequential([T.Linear(12, 10, True)])], (3, 20), CONVS | CHAIN, 0, 0),
    ("two Linears inside a nested Sequential", lambda T: [T.Linear(20, 12, True), T.Sequential([T.Linear(12, 10, True), T.ReLU(), T.Linear(10, 4, True)])], (3, 20),
     0, 1, 0),
    # (a Linear takes [batch, in_features] alone, so Flatten(0) never leads into one, and Flatten(2) only with a Flatten(1) behind it)
    ("Flatten(2) then Flatten(1) behind a conv", lambda T: [_c3(T, 1, 5), T.Flatten(2), T.Flatten(1)] + _lin_tail(T, 20), (2, 1, 2, 2), CONVS | CHAIN, 1, 0),
    ("an AvgPool in front of Flatten", lambda T: [_c3(T, 1, 6), T.AvgPool2d((2, 2), (2, 2)), T.Flatten(1)] + _lin_tail(T, 24), (2, 1, 4, 4), CONVS | CHAIN, 1, 0),
    ("a 129-channel conv in front of Flatten", lambda T: [_c3(T, 1, 129), T.Flatten(1)] + _lin_tail(T, 129 * 4), (2, 1, 2, 2), CONVS | CHAIN, 1, 0),
    ("a 1-channel conv on a 17 x 241 map", lambda T: [_c3(T, 1, 1), T.Flatten(1)] + _lin_tail(T, 4097), (1, 1, 17, 241), CONVS | CHAIN, 1, 0),
    ("LINKS without CONVS on the CNN", None, (2, 1, 8, 8), 0, 1, 0),
    ("LINKS with CONVS but without CHAIN on the CNN", None, (2, 1, 8, 8), CONVS, 1, 0),
    ("a strided (weight-only) conv in front of Flatten", lambda T: [T.Conv2dReLU(1, 6, (3, 3), (2, 2), (1, 1)), T.Flatten(1)] + _lin_tail(T, 24), (2, 1, 4, 4),
     CONVS | CHAIN, 1, 0),
    ("two pools in front of Flatten", lambda T: [_c3(T, 1, 6), T.MaxPool2d((2, 2)), T.MaxPool2d((2, 2)), T.Flatten(1)] + _lin_tail(T, 6), (2, 1, 4, 4), CONVS | CHAIN, 1, 0),
]


@pytest.mark.parametrize("variant", NO_LINKS, ids=[v[0].replace(" ", "_") for v in NO_LINKS])
def test_boundaries_that_are_no_link_run_as_before(variant):
    import taper_amd as T
    name, layers, shape, flags, links, links_plain = variant
    rng = np.random.default_rng(sum(map(ord, name)))
    model = _randomize(_cnn(T) if "on the CNN" in name else T.Sequential(layers(T)), rng, 0.3)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    linked, plain = _linked_and_plain(model, calib, flags, links)
    assert plain.chain_links() == links_plain and linked.storage_bytes() == plain.storage_bytes()
    _assert_same_forward(linked, plain, rng.standard_normal(shape).astype(f32), shape)


def test_flag_refusals_and_model_refusals():
    import taper_amd as T
    rng = np.random.default_rng(77)
    model = _randomize(_cnn(T), rng)
    shape = (2, 1, 8, 8)
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    dropout, flat = T.Sequential([T.Linear(20, 12, True), T.Dropout(0.5), T.Linear(12, 10, True)]), T.Tensor(np.zeros((2, 20), f32), (2, 20))
    T.Device.sync()
    before = _pool_in_use()
    for flags in (8, -1, 8 | LINKS):
        with pytest.raises(T.TaperError, match="unknown flag bits"):
            _twin(model, x, flags)
    for flags in (CHAIN | LINKS, CHAIN | LINKS | PER_CHANNEL):
        with pytest.raises(T.TaperError, match="TP_QSTATIC_CHAIN needs TP_QSTATIC_CONVS"):
            _twin(model, x, flags)
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static_linked(flat)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        model.quantize_static_linked([])
    assert _pool_in_use() == before
    q = model.quantize_static_linked(x)                  # and the next valid call succeeds
    assert q.chain_links() == 3 and q.act_scales().shape == (4,)
    held = _pool_in_use()
    plain = model.quantize_static_chain(x)
    wrong = (2, 1, 12, 12)                               # a larger map: Flatten gives the Linear 54 features
    for twin in (plain, q):
        with pytest.raises(T.TaperError, match=r"QuantizedLinear: input must be \[batch, in_features\]"):
            twin(T.Tensor(np.zeros(wrong, f32), wrong))
    del plain
    assert _pool_in_use() == held                        # a forward refused halfway gives its buffers back
    assert q(x).data().shape == (2, 10)
