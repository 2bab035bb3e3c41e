"""Per-channel int8 weight scales on the GPU: th_quantize_int8_channels in both geometries, the three products that read one
{mw, sw} pair per output channel, and Module.quantize_static_per_channel, against the numpy restatement of tests/qperchan_ref.py.  The
sums are exact int32 and the epilogue is four f32 operations rounded once each, so every comparison with the restatement is on bits; the
_pc calls run through the guard / NaN-fill harnesses of tests/test_gpu_qstatic.py, test_gpu_qconv.py and test_gpu_qchain.py."""
import ctypes as C

import numpy as np
import pytest

from tests import backends as B
from tests import margins
from tests import qconv_ref as Q
from tests import qperchan_ref as P
from tests import qstatic_ref as R
from tests import test_gpu_qchain as TCH
from tests import test_gpu_qconv as TC
from tests import test_gpu_qstatic as TL

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64
BPARAMS = TL.BPARAMS
_bits, _in_use, _lib, _pool_in_use = TC._bits, TC._in_use, TC._lib, TC._pool_in_use


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


class _PerChannel:
    """a Ctx whose call() sends the three per-tensor products to their per-channel twins: the older tests' harnesses, unchanged, then
    exercise the _pc entry points (same arguments; d_wparams holds a pair per channel)"""
    NAMES = {"th_linear_q8q8_fwd": "th_linear_q8q8_fwd_pc", "th_conv2d_q8q8_fwd": "th_conv2d_q8q8_fwd_pc",
             "th_conv2d_q8q8_fwd_codes": "th_conv2d_q8q8_fwd_codes_pc"}

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def call(self, name, *args):
        return self._ctx.call(self.NAMES.get(name, name), *args)


@pytest.fixture(scope="module")
def pc(ctx):
    return _PerChannel(ctx)


def int_pairs(n):
    """sx = 1 goes with these: mw = 0, sw[n] = n + 1 -- pure integers, so a pair that reaches another column shows"""
    return np.stack([np.zeros(n, f32), np.arange(1, n + 1, dtype=f32)], axis=1)


def float_pairs(n):
    """a float codec that differs in every channel"""
    i = np.arange(n, dtype=f32)
    return np.stack([f32(-0.31) + f32(0.003) * i, f32(0.0024) * (f32(1) + f32(0.01) * i)], axis=1).astype(f32)


PAIR_SETS = [(1.0, int_pairs), (0.0173, float_pairs)]      # (sx, pairs)
FORMS = ((0, 0), (1, 0), (1, 1), (0, 1))                   # (bias, relu)


# ---------------------------------------------------------------- 1: the codec
CODEC_SHAPES = [(1, 1), (3, 17), (10, 784), (33, 5), (128, 1152), (260, 32)]      # (channels, len)


def _codec_input(channels, ln):
    """[channels, len] without -0.0; from three channels on: channel 0 constant (the +-0.1 widening), channel 1 NaN and +-inf among finite
    values, channel 2 nothing finite"""
    rng = np.random.default_rng(channels * 1000 + ln)
    a = (rng.standard_normal((channels, ln)) * (1 + np.arange(channels))[:, None]).astype(f32)
    a[a == 0] = f32(0.5)
    if channels >= 3:
        a[0] = f32(0.75)
        a[1, 0], a[1, ln // 2], a[1, ln - 1] = np.nan, np.inf, -np.inf
        a[2, ::3], a[2, 1::3], a[2, 2::3] = np.nan, np.inf, -np.inf
    return a


def _codec_call(ctx, layout, channels, ln, chan_stride, elem_stride):
    """one th_quantize_int8_channels call on the array as it lies in memory: guard bytes around the codes and guard words around the pairs
    must come back untouched, pool bytes in use unchanged"""
    n = channels * ln
    qbuf = ctx.upload(np.concatenate([np.full(4 * GUARD, 0xA5, np.uint8), np.full(n, 0x55, np.uint8), np.full(4 * GUARD, 0xA5, np.uint8)]))
    pbuf = ctx.upload(np.full(2 * channels + 2 * GUARD, TL.GUARD_BITS, np.uint32))
    dx = ctx.upload(np.ascontiguousarray(layout, f32))
    before = _in_use(ctx)
    ctx.call("th_quantize_int8_channels", dx, channels, ln, chan_stride, elem_stride, qbuf.offset(4 * GUARD), pbuf.offset(4 * GUARD))
    assert _in_use(ctx) == before
    qraw, praw = ctx.download(qbuf, (n + 8 * GUARD,), np.uint8), ctx.download(pbuf, (2 * channels + 2 * GUARD,), np.uint32)
    assert (qraw[:4 * GUARD] == 0xA5).all() and (qraw[4 * GUARD + n:] == 0xA5).all(), "bytes around the codes were written"
    assert (praw[:GUARD] == TL.GUARD_BITS).all() and (praw[GUARD + 2 * channels:] == TL.GUARD_BITS).all(), "words around the pairs were written"
    return qraw[4 * GUARD:4 * GUARD + n].view(np.int8).reshape(np.shape(layout)), praw[GUARD:GUARD + 2 * channels].view(f32).reshape(channels, 2)


@pytest.mark.parametrize("channels,ln", CODEC_SHAPES, ids=lambda v: str(v))
def test_codec_rows_and_columns_are_the_storage_codec_of_every_channel(ctx, channels, ln):
    a = _codec_input(channels, ln)
    ref_q, ref_p = P.pack_channels(a, 0)
    if channels >= 3:
        assert ref_p[0, 0] == f32(0.75) - f32(0.1) and np.isinf(ref_p[2]).all() and (ref_q[2] == -128).all()
        assert ref_q[1, ln // 2] == 127 and ref_q[1, ln - 1] == -128 and np.isfinite(ref_p[1]).all()
    q, p = _codec_call(ctx, a, channels, ln, ln, 1)                       # rows: a Linear weight [out, in]
    np.testing.assert_array_equal(q, ref_q)
    np.testing.assert_array_equal(p, ref_p)
    q, p = _codec_call(ctx, a.T, channels, ln, 1, channels)               # columns: [len][channels], a Conv2d buffer as the float kernels read it
    np.testing.assert_array_equal(q, ref_q.T)
    np.testing.assert_array_equal(p, ref_p)


@pytest.mark.parametrize("n", [1, 17, 5000])
def test_one_channel_is_th_quantize_int8_bit_for_bit(ctx, n):
    x = _codec_input(1, n)
    x[0, n // 2] = np.inf
    q, p = _codec_call(ctx, x, 1, n, n, 1)
    dq, dp = ctx.upload(np.full(n, 0x55, np.uint8)), ctx.empty(2)
    ctx.call("th_quantize_int8", ctx.upload(x), dq, n, dp)
    np.testing.assert_array_equal(q.reshape(-1), ctx.download(dq, (n,), np.int8))
    np.testing.assert_array_equal(_bits(p.reshape(-1)), _bits(ctx.download(dp, (2,))))
    q2, p2 = _codec_call(ctx, x, 1, n, 1, 1)                              # (with one channel, chan_stride has nothing to say)
    np.testing.assert_array_equal(q2, q)
    np.testing.assert_array_equal(_bits(p2), _bits(p))


def test_codec_refusals_name_the_function_and_the_next_call_succeeds(ctx):
    hip = _lib()
    a = _codec_input(4, 6)
    dx, dq, dp = ctx.upload(a), ctx.upload(np.full(24, 0x55, np.uint8)), ctx.upload(np.full(8, TL.GUARD_BITS, np.uint32))
    good = dict(x=int(dx), ch=4, ln=6, cs=6, es=1, q=int(dq), p=int(dp))

    def call(**kw):
        g = dict(good, **kw)
        return hip.th_quantize_int8_channels(ctx.h, g["x"], g["ch"], g["ln"], g["cs"], g["es"], g["q"], g["p"])

    before = _in_use(ctx)
    for what, kw in (("null input", dict(x=None)), ("null codes", dict(q=None)), ("null pairs", dict(p=None)), ("channels 0", dict(ch=0)), ("len 0", dict(ln=0)),
                     ("negative len", dict(ln=-3)), ("rows with a pitch", dict(cs=8)), ("columns with another stride", dict(cs=1, es=5)),
                     ("both strides 1", dict(cs=1, es=1)), ("a transposed pitch", dict(cs=6, es=4))):
        assert call(**kw) != 0 and b"th_quantize_int8_channels" in hip.th_last_error(), what
    assert hip.th_quantize_int8_channels(None, *[good[f] for f in ("x", "ch", "ln", "cs", "es", "q", "p")]) != 0
    assert _in_use(ctx) == before
    assert (ctx.download(dq, (24,), np.uint8) == 0x55).all() and (ctx.download(dp, (8,), np.uint32) == TL.GUARD_BITS).all(), "a refused call wrote"
    assert call() == 0
    ref_q, ref_p = P.pack_channels(a, 0)
    np.testing.assert_array_equal(ctx.download(dq, (4, 6), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(dp, (4, 2)), ref_p)


# ---------------------------------------------------------------- 2: the Linear product
def _switch():
    return max(b for b in range(1, 4097) if TL.plan(b, 64, 64)["skinny"])


LINEAR_N, LINEAR_K = (1, 31, 33, 129), (1, 17, 64, 784)


def _linear_batches():
    s = _switch()
    return (1, 5, s, s + 1)


def test_linear_case_table_stands_on_both_sides_of_the_switch():
    s = _switch()
    assert [TL.plan(b, 64, 33)["skinny"] for b in (1, 5, s, s + 1)] == [1, 1, 1, 0]
    assert TL.plan(s + 1, 64, 129)["tiles_n"] == 2 and TL.plan(s + 1, 64, 129)["tiles_m"] == -(-(s + 1) // 128) and TL.plan(s, 64, 33)["tiles_n"] == 2


@pytest.mark.parametrize("K", LINEAR_K)
@pytest.mark.parametrize("N", LINEAR_N)
@pytest.mark.parametrize("b", range(4), ids=("B1", "B5", "switch", "switch+1"))
def test_linear_product_is_the_reference_bit_for_bit(pc, b, N, K):
    M = _linear_batches()[b]
    i = 16 * b + 4 * LINEAR_N.index(N) + LINEAR_K.index(K)
    qx, qw, qb = TL._operands(M, N, K, seed=M * 7919 + N * 31 + K)
    rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    pitch_x = TL._up16(K) + 16 * (i % 3)
    pitch_w = -(-K // 64) * 64 if i % 2 else TL._up16(K)
    for sx, pairs in PAIR_SETS:
        wp = pairs(N)
        for bias, relu in FORMS:
            ref = P.linear_q8q8_pc(qx, sx, qw, wp, qb if bias else None, BPARAMS, relu)
            got = TL._product(pc, qx, rs, sx, qw, wp, qb if bias else None, BPARAMS, relu, pitch_x, pitch_w)
            np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str(((M, N, K), sx, "bias", bias, "relu", relu)))


# ---------------------------------------------------------------- 3: the conv products
CONV_CASES = [TC.CASES[i] for i in (0, 1, 2, 3, 6, 7, 8, 9)]
CONV_IDS = [TC.IDS[i] for i in (0, 1, 2, 3, 6, 7, 8, 9)]
CODES_CASES = [c for c in CONV_CASES if c[4] <= 128]
CODES_IDS = [i for c, i in zip(CONV_CASES, CONV_IDS) if c[4] <= 128]


def test_conv_case_table_reaches_every_form_and_edge():
    rows = [(c, TC.plan(*c)) for c in CONV_CASES]
    assert {p["nt"] for _, p in rows} == {1, 2, 4} and {p["nt"] for c, p in rows if c[4] <= 128} == {1, 2, 4}
    assert {c[4] for c, _ in rows} >= {1, 31, 33, 127, 128, 129, 260}
    assert any(p["tiles_n"] == 3 for _, p in rows) and any(p["tiles_n"] == 2 for _, p in rows)
    px = [(c[0] * p["h_out"] * p["w_out"], p["h_out"] * p["w_out"], p["tile_m"]) for c, p in rows]
    assert any(m % t == 1 and m > t for m, _, t in px), "a pixel count one past a tile"
    assert any(per < t and m > per for m, per, t in px), "a tile that spans images"
    assert all(TC.plan(*c)["tiles_n"] == 1 for c in CODES_CASES)


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv_product_is_the_reference_bit_for_bit(pc, case):
    n, c_in, h, w, c_out, k, s, p = case
    i = TC.CASES.index(case)
    qx, qw, qb = TC._operands(n, c_in, h, w, c_out, k, seed=1000 + i)
    pitch = Q.cpitch(c_in) + 16 * (i % 2)
    for sx, pairs in PAIR_SETS:
        wp = pairs(c_out)
        for bias, relu in FORMS:
            ref = P.conv_q8q8_pc(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu)
            got = TC._product(pc, qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, pitch)
            assert not np.isnan(ref).any()
            np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str((case, sx, "bias", bias, "relu", relu)))


@pytest.mark.parametrize("case", CODES_CASES, ids=CODES_IDS)
def test_conv_codes_padding_and_pixel_sums_are_the_reference(pc, case):
    n, c_in, h, w, c_out, k, s, p = case
    qx, qw, qb = TC._operands(n, c_in, h, w, c_out, k, seed=2000 + TC.CASES.index(case))
    # both pair sets with and without bias and ReLU; pixel sums asked for or not; the tightest pitch and looser ones
    extras = ((1, 0), (0, 0), (1, 32), (0, 16))
    for sx, pairs in PAIR_SETS:
        wp = pairs(c_out)
        for (bias, relu), (want_sums, extra) in zip(FORMS, extras):
            y = P.conv_q8q8_pc(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu)
            sy = f32(R.act_scale_of(y) * f32(0.6))          # the next layer's scale: the outer 40 % of the range saturates
            pitch_y = Q.cpitch(c_out) + extra
            ref_q, ref_ps = P.conv_q8q8_codes_pc(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, sy, pitch_y)
            got_q, got_ps = TCH._codes_call(pc, qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, sy, pitch_y, want_sums)
            what = str((case, sx, "bias", bias, "relu", relu, "pitch", pitch_y))
            np.testing.assert_array_equal(got_q[..., :c_out], ref_q[..., :c_out], err_msg=what)
            assert not got_q[..., c_out:].any(), "padding bytes must be 0: " + what
            if want_sums:
                np.testing.assert_array_equal(got_ps, ref_ps, err_msg=what)
            else:
                assert (got_ps == TCH.FILL).all(), "pixel sums were written although none were asked for"


# ---------------------------------------------------------------- 4: the tie to the per-tensor code
def test_one_pair_repeated_gives_the_per_tensor_twins_bits(ctx, pc):
    s = _switch()
    for sx, wp in TL.PARAMS:
        for M, N, K in ((5, 33, 784), (s + 1, 129, 64)):      # the skinny form and the 128 x 128 tiles
            qx, qw, qb = TL._operands(M, N, K, seed=M + N + K)
            rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
            a = TL._product(pc, qx, rs, sx, qw, P.same_pair(wp, N), qb, BPARAMS, 1, TL._up16(K), TL._up16(K))
            b = TL._product(ctx, qx, rs, sx, qw, wp, qb, BPARAMS, 1, TL._up16(K), TL._up16(K))
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=str((M, N, K)))
        for case in (TC.CASES[1], TC.CASES[3], TC.CASES[8], TC.CASES[9]):      # NT = 1, 2, 4, and three channel tiles
            n, c_in, h, w, c_out, k, st, p = case
            qx, qw, qb = TC._operands(n, c_in, h, w, c_out, k, seed=c_out)
            a = TC._product(pc, qx, sx, qw, P.same_pair(wp, c_out), qb, BPARAMS, st, p, 1, Q.cpitch(c_in))
            b = TC._product(ctx, qx, sx, qw, wp, qb, BPARAMS, st, p, 1, Q.cpitch(c_in))
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=str(case))
            if c_out > 128:
                continue
            sy = f32(R.act_scale_of(b) * f32(0.6))
            qa, sa = TCH._codes_call(pc, qx, sx, qw, P.same_pair(wp, c_out), qb, BPARAMS, st, p, 1, sy, Q.cpitch(c_out), True)
            qb_, sb = TCH._codes_call(ctx, qx, sx, qw, wp, qb, BPARAMS, st, p, 1, sy, Q.cpitch(c_out), True)
            np.testing.assert_array_equal(qa, qb_, err_msg=str(case))
            np.testing.assert_array_equal(sa, sb, err_msg=str(case))


def test_a_layer_wider_than_one_workgroup_is_refused_by_the_new_name(ctx):
    hip = _lib()
    n, c_in, h, w, k = 1, 16, 5, 5, (3, 3)
    qx, qw, _ = TC._operands(n, c_in, h, w, 129, k, seed=5)
    dx, dw = ctx.upload(Q.nhwc(qx, 16).view(np.uint8)), ctx.upload(Q.pack_weight(qw, 16).view(np.uint8))
    dps = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32))
    dsx, dwp, dsy = ctx.upload(np.array([1.0], f32)), ctx.upload(int_pairs(129)), ctx.upload(np.array([90000.0], f32))
    dq, dsum = ctx.upload(np.full(9 * 144 + 64, TCH.FILL, np.uint8)), ctx.upload(np.full(9, TCH.FILL, np.int32))

    def call(co, cpy, wp=int(dwp)):
        return hip.th_conv2d_q8q8_fwd_codes_pc(ctx.h, int(dx), 16, int(dps), int(dsx), n, c_in, h, w, int(dw), co, 3, 3, 1, 1, 0, 0, wp, None, None, 0,
                                               int(dsy), int(dq), cpy, int(dsum))

    before = _in_use(ctx)
    assert call(129, 144) != 0
    assert b"th_conv2d_q8q8_fwd_codes_pc" in hip.th_last_error() and b"129" in hip.th_last_error()
    assert call(128, 128, None) != 0 and b"th_conv2d_q8q8_fwd_codes_pc" in hip.th_last_error()
    assert hip.th_conv2d_q8q8_fwd_pc(ctx.h, int(dx), 24, int(dps), int(dsx), n, c_in, h, w, int(dw), 128, 3, 3, 1, 1, 0, 0, int(dwp), None, None, 0, int(dq)) != 0
    assert b"th_conv2d_q8q8_fwd_pc" in hip.th_last_error()
    assert hip.th_linear_q8q8_fwd_pc(ctx.h, int(dx), 24, int(dps), int(dsx), 1, 16, int(dw), 16, 4, int(dwp), None, None, 0, int(dq)) != 0
    assert b"th_linear_q8q8_fwd_pc" in hip.th_last_error()
    assert _in_use(ctx) == before
    assert (ctx.download(dq, (9 * 144 + 64,), np.uint8) == TCH.FILL).all(), "a refused call wrote"
    assert call(128, 128) == 0                           # the next call succeeds: exactly the limit
    ref_q, ref_ps = P.conv_q8q8_codes_pc(qx, 1.0, qw[:128], int_pairs(128), None, None, (1, 1), (0, 0), False, 90000.0, 128)
    np.testing.assert_array_equal(ctx.download(dq, (1, 3, 3, 128), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(dsum, (1, 3, 3), np.int32), ref_ps)
    assert len(np.unique(ref_q)) > 8


# ---------------------------------------------------------------- 5: batch independence
def test_a_rows_and_an_images_result_do_not_depend_on_the_batch(pc):
    M, N, K = _switch() + 1, 33, 100                      # the whole batch takes the 128 x 128 tiles, a row alone the skinny form
    qx, qw, qb = TL._operands(M, N, K, seed=91)
    rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    sx, wp = 0.0173, float_pairs(N)
    whole = TL._product(pc, qx, rs, sx, qw, wp, qb, BPARAMS, 0, 112, 128)
    for b in (0, 130, M - 1):
        alone = TL._product(pc, qx[b:b + 1], rs[b:b + 1], sx, qw, wp, qb, BPARAMS, 0, 112, 128)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[b]), err_msg=f"row {b} alone")
    n, c_in, h, w, c_out, k, s, p = 5, 15, 7, 11, 32, (3, 3), (1, 1), (1, 1)      # 77 pixels an image: every image starts at another place of a tile
    qx, qw, qb = TC._operands(n, c_in, h, w, c_out, k, seed=77)
    wp = float_pairs(c_out)
    whole = TC._product(pc, qx, sx, qw, wp, qb, BPARAMS, s, p, 1, 16)
    sy = f32(R.act_scale_of(whole) * f32(0.6))
    whole_q, whole_ps = TCH._codes_call(pc, qx, sx, qw, wp, qb, BPARAMS, s, p, 1, sy, 32, True)
    for b in range(n):
        alone = TC._product(pc, qx[b:b + 1], sx, qw, wp, qb, BPARAMS, s, p, 1, 16)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[b]), err_msg=f"image {b} alone")
        q1, ps1 = TCH._codes_call(pc, qx[b:b + 1], sx, qw, wp, qb, BPARAMS, s, p, 1, sy, 32, True)
        np.testing.assert_array_equal(q1[0], whole_q[b], err_msg=f"image {b} alone")
        np.testing.assert_array_equal(ps1[0], whole_ps[b], err_msg=f"image {b} alone")


# ---------------------------------------------------------------- 6: the twins
def _assert_pairs(got, ref):
    got = np.asarray(got, f32)
    assert got.shape == np.shape(ref)
    np.testing.assert_array_equal(_bits(got), _bits(np.asarray(ref, f32)))


@pytest.fixture(scope="module")
def mlp_twins():
    import taper_amd as T
    rng = np.random.default_rng(21)
    model, vals = TL._mlp(rng)
    calib = [T.Tensor(c, (32, 784)) for c in (rng.standard_normal((32, 784)).astype(f32), (2.5 * rng.standard_normal((32, 784))).astype(f32))]
    T.Tape.reset()
    q = model.quantize_static_per_channel(calib)
    return dict(model=model, vals=vals, q=q, tape_len=T.Tape.len(), per_tensor=model.quantize_static(calib))


def test_mlp_twin_packs_every_row_alone_and_keeps_the_per_tensor_scales(mlp_twins):
    q, vals, old = mlp_twins["q"], mlp_twins["vals"], mlp_twins["per_tensor"]
    assert mlp_twins["tape_len"] == 0 and q.chain_links() == 0
    np.testing.assert_array_equal(_bits(q.act_scales()), _bits(old.act_scales()))
    ts = q.tensors()
    assert [q.channel_layout(i) for i in range(4)] == [(128, 784, 1), (1, 0, 1), (10, 128, 1), (1, 0, 1)]
    assert [old.channel_layout(i) for i in range(4)] == [(1, 0, 1)] * 4
    for (kind, codes, pairs), v, rows in zip(ts, vals, (128, None, 10, None)):
        assert kind == "int8"
        if rows:
            ref_q, ref_p = P.pack_channels(v.reshape(rows, -1), 0)
            assert isinstance(pairs, np.ndarray) and pairs.shape == (rows, 2)
        else:
            ref_q, ref_p = R.pack(v)
            assert isinstance(pairs, tuple)
        np.testing.assert_array_equal(codes, ref_q.reshape(-1))
        _assert_pairs(pairs, ref_p)
    for (_, c1, p1), (_, c2, p2) in zip(ts[1::2], old.tensors()[1::2]):      # the biases: the per-tensor twin's
        np.testing.assert_array_equal(c1, c2)
        _assert_pairs(p1, p2)
    step = _lib().th_qlinear_i8_kstep()
    padded = 128 * (-(-784 // step) * step) + 10 * (-(-128 // step) * step)
    assert q.storage_bytes() == padded + 128 + 10 + 8 * (128 + 10) + 8 * 2 + 4 * 2
    assert old.storage_bytes() == padded + 128 + 10 + 8 * 4 + 4 * 2


def test_mlp_twin_forward_is_the_reference_chain_bit_for_bit(mlp_twins):
    import taper_amd as T
    q = mlp_twins["q"]
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2) = q.tensors()
    scales = q.act_scales()
    x = np.random.default_rng(22).standard_normal((37, 784)).astype(f32)
    T.Tape.reset()
    before = _pool_in_use()
    y = q(T.Tensor(x, (37, 784)).requires_grad())
    assert T.Tape.len() == 0 and y.tape_node() == 0
    got = y.data()
    del y
    assert _pool_in_use() == before
    h = P.linear_q8q8_pc(R.quantize_act(x, scales[0])[0], scales[0], w1.reshape(128, 784), p1, b1, q1, relu=True)
    ref = P.linear_q8q8_pc(R.quantize_act(h, scales[1])[0], scales[1], w2.reshape(10, 128), p2, b2, q2)
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    assert not np.array_equal(_bits(got), _bits(mlp_twins["per_tensor"](T.Tensor(x, (37, 784))).data()))      # another codec: other bits
    for b in (0, 17, 36):
        alone = q(T.Tensor(x[b:b + 1], (1, 784))).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(got[b]), err_msg=f"row {b} alone")
    big = np.random.default_rng(23).standard_normal((_switch() + 1, 784)).astype(f32)      # the 128 x 128 tiles
    np.testing.assert_array_equal(_bits(q(T.Tensor(big, big.shape)).data()[:3]), _bits(q(T.Tensor(big[:3], (3, 784))).data()))


@pytest.fixture(scope="module")
def cnn_twins():
    import taper_amd as T
    rng = np.random.default_rng(51)
    model, layers, vals = TC._cnn(rng)
    calib = [T.Tensor(c, TC.SHAPE) for c in (rng.uniform(0, 1, TC.SHAPE).astype(f32), (1.5 * rng.standard_normal(TC.SHAPE)).astype(f32))]
    T.Tape.reset()
    chain = model.quantize_static_per_channel(calib)
    tape_len = T.Tape.len()
    return dict(model=model, vals=vals, chain=chain, tape_len=tape_len, plain=model.quantize_static_per_channel(calib, convs=True, chain=False),
                linear_only=model.quantize_static_per_channel(calib, convs=False, chain=False), per_tensor=model.quantize_static_chain(calib),
                calib=calib)


def test_cnn_twin_packs_every_effective_channel_alone(cnn_twins):
    chain, plain, old, vals = cnn_twins["chain"], cnn_twins["plain"], cnn_twins["per_tensor"], cnn_twins["vals"]
    assert cnn_twins["tape_len"] == 0
    assert chain.chain_links() == old.chain_links() == 1 and plain.chain_links() == 0
    for tw in (chain, plain, cnn_twins["linear_only"]):
        np.testing.assert_array_equal(_bits(tw.act_scales()), _bits(old.act_scales())[-len(tw.act_scales()):])
    assert cnn_twins["linear_only"].act_scales().shape == (1,) and chain.act_scales().shape == (3,)
    assert [chain.channel_layout(i) for i in range(6)] == [(4, 1, 4), (1, 0, 1), (8, 1, 8), (1, 0, 1), (10, 32, 1), (1, 0, 1)]
    assert [cnn_twins["linear_only"].channel_layout(i) for i in range(6)] == [(1, 0, 1)] * 4 + [(10, 32, 1), (1, 0, 1)]      # weight-only convs: one pair
    geometry = ((4, 1), None, (8, 4), None, None, None)
    ta, tb = chain.tensors(), plain.tensors()
    for i, ((kind, codes, pairs), v, g) in enumerate(zip(ta, vals, geometry)):
        if g:
            ref_q, ref_p = P.taper_pack_channels(v, g[0], g[1], (3, 3))
        elif i == 4:
            ref_q, ref_p = P.pack_channels(v.reshape(10, 32), 0)
        else:
            ref_q, ref_p = R.pack(v)
        np.testing.assert_array_equal(codes, np.asarray(ref_q).reshape(-1), err_msg=str(i))
        _assert_pairs(pairs, ref_p)
        np.testing.assert_array_equal(codes, tb[i][1])
        _assert_pairs(pairs, tb[i][2])
    assert chain.storage_bytes() == plain.storage_bytes() == old.storage_bytes() + 8 * (4 + 8 + 10 - 3)


def _cnn_ref_chain(ts, scales, x):
    """tests/test_gpu_qconv.py's reference forward with a pair per output channel of every weight"""
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2), (_, w3, p3), (_, b3, q3) = ts
    h = P.conv_q8q8_pc(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 4, 1, (3, 3)), p1, b1, q1, relu=True)
    h = Q.max_pool(h, (2, 2), (2, 2))
    h = P.conv_q8q8_pc(Q.quantize_act_nchw(h, scales[1])[0], scales[1], Q.taper_weight(w2, 8, 4, (3, 3)), p2, b2, q2, pad=(1, 1), relu=True)
    h = Q.max_pool(h, (2, 2), (2, 2)).reshape(x.shape[0], -1)
    return P.linear_q8q8_pc(R.quantize_act(h, scales[2])[0], scales[2], w3.reshape(10, 32), p3, b3, q3)


def test_cnn_twin_forward_is_the_reference_chain_and_the_chain_changes_no_bit(cnn_twins):
    import taper_amd as T
    chain, plain = cnn_twins["chain"], cnn_twins["plain"]
    x = np.random.default_rng(52).standard_normal(TC.SHAPE).astype(f32)
    far = (3 * 1.5 * 4 * np.sign(x)).astype(f32)          # beyond the calibration range: the first codes saturate
    far[:, :, :, ::3] = x[:, :, :, ::3]
    T.Tape.reset()
    before = _pool_in_use()
    for data in (x, far):
        y = chain(T.Tensor(data, TC.SHAPE).requires_grad())
        assert T.Tape.len() == 0 and y.tape_node() == 0
        got = y.data()
        del y
        assert _pool_in_use() == before
        np.testing.assert_array_equal(_bits(got), _bits(_cnn_ref_chain(chain.tensors(), chain.act_scales(), data)))
        np.testing.assert_array_equal(_bits(got), _bits(plain(T.Tensor(data, TC.SHAPE)).data()))
    got = chain(T.Tensor(x, TC.SHAPE)).data()
    for b in (0, 3, 7):
        alone = chain(T.Tensor(x[b:b + 1], (1,) + TC.SHAPE[1:])).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(got[b]), err_msg=f"image {b} alone")
    assert _pool_in_use() == before


@pytest.mark.parametrize("name", ["cnn_reference-b3", "cnn_simple-b2"])
def test_chained_per_channel_twin_is_the_unchained_one_bit_for_bit(name):
    import taper_amd as T
    build, shape, links = TCH.MODELS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    model = build(rng)
    calib = [T.Tensor(a, shape) for a in (rng.uniform(0, 1, shape).astype(f32), (1.5 * rng.standard_normal(shape)).astype(f32))]
    T.Tape.reset()
    chain, plain = model.quantize_static_per_channel(calib), model.quantize_static_per_channel(calib, chain=False)
    old = model.quantize_static_chain(calib)
    assert T.Tape.len() == 0
    assert chain.chain_links() == links == old.chain_links() and plain.chain_links() == 0
    np.testing.assert_array_equal(_bits(chain.act_scales()), _bits(old.act_scales()))
    np.testing.assert_array_equal(_bits(plain.act_scales()), _bits(old.act_scales()))
    assert chain.storage_bytes() == plain.storage_bytes() > old.storage_bytes()
    params = model.parameters()
    for i, ((_, c1, p1), (_, c2, p2), (_, c3, p3)) in enumerate(zip(chain.tensors(), plain.tensors(), old.tensors())):
        np.testing.assert_array_equal(c1, c2)
        _assert_pairs(p1, p2)
        shp = tuple(params[i].shape())
        if len(shp) == 1:                                 # a bias: the per-tensor twin's
            np.testing.assert_array_equal(c1, c3)
            _assert_pairs(p1, p3)
            continue
        v = params[i].data().reshape(-1)
        ref_q, ref_p = P.taper_pack_channels(v, shp[0], shp[1], shp[2:]) if len(shp) == 4 else P.pack_channels(v.reshape(shp), 0)
        assert chain.channel_layout(i) == ((shp[0], 1, shp[0]) if len(shp) == 4 else (shp[0], shp[1], 1))
        np.testing.assert_array_equal(c1, np.asarray(ref_q).reshape(-1), err_msg=str(i))
        _assert_pairs(p1, ref_p)
    x = rng.standard_normal(shape).astype(f32)
    before = _pool_in_use()
    got, ref = chain(T.Tensor(x, shape)).data(), plain(T.Tensor(x, shape)).data()
    assert _pool_in_use() == before
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    for b in (0, shape[0] - 1):
        alone = chain(T.Tensor(x[b:b + 1], (1,) + shape[1:])).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(ref[b]), err_msg=f"image {b} alone")


def test_a_grouped_and_a_1x1_conv_stay_per_tensor_inside_the_twin():
    import taper_amd as T
    rng = np.random.default_rng(61)
    front = [T.Conv2d(4, 8, (3, 3), None, (1, 1), None, 2), T.ReLU(), T.Conv2d(8, 6, (1, 1)), T.Conv2dReLU(6, 6, (5, 5), (2, 2), (2, 2)), T.Flatten(1)]
    lin = T.Linear(6 * 3 * 3, 10, True)
    model, prefix = T.Sequential(front + [lin]), T.Sequential(front)
    for p in model.parameters():
        p.set_data((0.3 * rng.standard_normal(p.numel())).astype(f32))
    shape = (3, 4, 6, 6)
    imgs, calib = rng.standard_normal(shape).astype(f32), T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    q, wo = model.quantize_static_per_channel(calib), model.quantize("int8")
    scales, ts = q.act_scales(), q.tensors()
    assert scales.shape == (1,) and len(ts) == 8 and q.chain_links() == 0      # the Linear's scale alone: none of the convs is static
    assert [q.channel_layout(i) for i in range(8)] == [(1, 0, 1)] * 6 + [(10, 54, 1), (1, 0, 1)]
    for (k1, c1, p1), (k2, c2, p2) in zip(ts[:6], wo.tensors()[:6]):
        assert k1 == k2 == "int8" and isinstance(p1, tuple)
        np.testing.assert_array_equal(c1, c2)
        _assert_pairs(p1, p2)
    feat = prefix.quantize("int8").forward(T.Tensor(imgs, shape)).data()      # the weight-only twin of the same prefix
    (_, w, wp), (_, b, bp) = ts[6:]
    ref = P.linear_q8q8_pc(R.quantize_act(feat.reshape(3, -1), scales[0])[0], scales[0], w.reshape(10, 54), wp, b, bp)
    np.testing.assert_array_equal(_bits(q(T.Tensor(imgs, shape)).data()), _bits(ref))


def test_qat_layers_deploy_as_their_inner_layers():
    import taper_amd as T
    rng = np.random.default_rng(63)
    shape = (4, 3, 8, 8)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    plain = T.Sequential([T.Conv2dReLU(3, 8, (3, 3), None, (1, 1), seed=3), T.MaxPool2d((2, 2), (2, 2)), T.Conv2dReLU(8, 8, (3, 3), None, (1, 1), seed=5),
                          T.Flatten(1), T.Linear(8 * 16, 10, True, seed=4)])
    qat_model = T.Sequential([T.QATConv2d(3, 8, (3, 3), None, (1, 1), relu=True, seed=3), T.MaxPool2d((2, 2), (2, 2)),
                              T.QATConv2d(8, 8, (3, 3), None, (1, 1), relu=True, seed=5), T.Flatten(1), T.QATLinear(8 * 16, 10, True, seed=4)])
    ref = plain.quantize_static_per_channel(calib)
    T.qat.enable()
    try:
        T.Tape.reset()
        q = qat_model.quantize_static_per_channel(calib)
        assert T.Tape.len() == 0
    finally:
        T.qat.disable()
    assert q.chain_links() == 1 and q.act_scales().shape == (3,)
    np.testing.assert_array_equal(_bits(q.act_scales()), _bits(ref.act_scales()))
    for i, ((_, c1, p1), (_, c2, p2)) in enumerate(zip(q.tensors(), ref.tensors())):
        assert q.channel_layout(i) == ref.channel_layout(i)
        np.testing.assert_array_equal(c1, c2)
        _assert_pairs(p1, p2)
    assert q.channel_layout(0) == (8, 1, 8) and q.channel_layout(4) == (10, 128, 1)
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    np.testing.assert_array_equal(_bits(q(x).data()), _bits(ref(x).data()))


def _static_ex(model, tensors, flags):
    """tp_module_quantize_static_ex itself -> (return code, handle)"""
    from taper_amd._lib import host
    arr = (C.c_void_p * max(len(tensors), 1))(*[t._h if t is not None else None for t in tensors])
    h = C.c_void_p()
    return host.tp_module_quantize_static_ex(model._h, arr, len(tensors), flags, C.byref(h)), h


def test_refusals_leak_nothing_and_the_next_call_succeeds():
    import taper_amd as T
    from taper_amd._lib import host
    shape = (2, 1, 12, 12)
    x = T.Tensor(np.zeros(shape, f32), shape)
    model, _, _ = TC._cnn(np.random.default_rng(64))
    dropout = T.Sequential([T.Conv2d(1, 4, (3, 3)), T.Dropout(0.5)])
    wide = T.Sequential([T.Conv2d(7282, 1, (3, 3), bias=False)])      # 7282 * 9 = 65538
    T.Device.sync()
    before = _pool_in_use()
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static_per_channel(x)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        model.quantize_static_per_channel([])
    with pytest.raises(T.TaperError, match="undefined calibration tensor"):
        model.quantize_static_per_channel([x, None])
    with pytest.raises(T.TaperError, match="65538"):
        wide.quantize_static_per_channel(T.Tensor(np.zeros((1, 7282, 3, 3), f32), (1, 7282, 3, 3)))
    for flags, what in ((2, b"TP_QSTATIC_CHAIN"), (2 | 4, b"TP_QSTATIC_CHAIN"), (8, b"unknown"), (-1, b"unknown")):
        rc, h = _static_ex(model, [x], flags)
        assert rc != 0 and not h.value and b"tp_module_quantize_static_ex" in host.tp_last_error() and what in host.tp_last_error(), flags
    assert _pool_in_use() == before
    q = model.quantize_static_per_channel(x)             # and the next valid call succeeds
    assert q.act_scales().shape == (3,) and q.chain_links() == 1
    # without the per-channel flag the call is the older entry points
    for flags, old in ((0, model.quantize_static(x)), (1, model.quantize_static_conv(x)), (3, model.quantize_static_chain(x))):
        rc, h = _static_ex(model, [x], flags)
        assert rc == 0
        tw = T.QuantizedModule(h.value)
        np.testing.assert_array_equal(_bits(tw.act_scales()), _bits(old.act_scales()))
        assert tw.chain_links() == old.chain_links() and tw.storage_bytes() == old.storage_bytes()
        assert [tw.channel_layout(i) for i in range(6)] == [(1, 0, 1)] * 6
    # a per-channel tensor's pairs do not fit tp_qmodule_tensor's two floats
    two, qt = np.zeros(2, f32), C.c_int(-1)
    held = _pool_in_use()
    assert host.tp_qmodule_tensor(q._h, 0, None, two.ctypes.data, None) != 0 and b"tp_qmodule_tensor_params" in host.tp_last_error()
    codes = np.zeros(36, np.int8)
    assert host.tp_qmodule_tensor(q._h, 0, codes.ctypes.data, None, C.byref(qt)) == 0 and qt.value == 0      # codes and qtype as before
    np.testing.assert_array_equal(codes, q.tensors()[0][1])
    assert host.tp_qmodule_tensor(q._h, 1, None, two.ctypes.data, None) == 0                                  # a bias: one pair, as before
    n = C.c_size_t()
    assert host.tp_qmodule_tensor_params(q._h, 0, None, 0, C.byref(n)) == 0 and n.value == 4
    pairs = np.full((4, 2), 7, f32)
    assert host.tp_qmodule_tensor_params(q._h, 0, pairs.ctypes.data, 2, C.byref(n)) == 0 and n.value == 4      # a short buffer: the first two
    _assert_pairs(pairs[:2], q.tensors()[0][2][:2])
    assert (pairs[2:] == 7).all()
    assert host.tp_qmodule_tensor_params(q._h, 1, pairs.ctypes.data, 4, C.byref(n)) == 0 and n.value == 1
    _assert_pairs(pairs[0], two)
    assert host.tp_qmodule_tensor_params(q._h, 6, None, 0, C.byref(n)) != 0 and b"tp_qmodule_tensor_params" in host.tp_last_error()
    ch = C.c_size_t()
    assert host.tp_qmodule_tensor_channels(q._h, 6, C.byref(ch), C.byref(ch), C.byref(ch)) != 0 and b"tp_qmodule_tensor_channels" in host.tp_last_error()
    assert _pool_in_use() == held
    with pytest.raises(T.TaperError, match="in_channels"):      # a forward refused halfway gives its buffers back
        q(T.Tensor(np.zeros((2, 3, 12, 12), f32), (2, 3, 12, 12)))
    assert _pool_in_use() == held
    assert q(x).data().shape == (2, 10)


# ---------------------------------------------------------------- 7: accuracy on the device
@pytest.mark.parametrize("seed", range(5))
def test_per_channel_twin_recovers_the_small_rows(seed):
    """tests/test_qperchan_abi.py's construction set into a model (no bias: a per-tensor bias code would add its own error to the small
    columns) and calibrated on the test's own inputs: the per-channel twin's worst small-row column error is at most a tenth of
    quantize_static's.  The restatement alone gives a factor of 58 to 106 on these seeds (CPU)."""
    import taper_amd as T
    x, w, _ = P.scaled_rows_layer(seed)
    model = T.Sequential([T.Linear(100, 40, False)])
    model.parameters()[0].set_data(w)
    xt = T.Tensor(x, x.shape)
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    small = np.arange(40) % 8 >= 5
    norm = np.abs(y64).max(axis=0)[small]
    errs = {}
    for name, twin in (("per_tensor", model.quantize_static(xt)), ("per_channel", model.quantize_static_per_channel(xt))):
        y = twin(xt).data()
        errs[name] = P.small_row_error(y, y64)
        rec = margins.check(f"small_rows_{name}", y[:, small] / norm, y64[:, small] / norm, None, test="test_per_channel_twin_recovers_the_small_rows")
        assert abs(rec["max_abs_err"] - errs[name]) <= 1e-9
    T.Tape.reset()
    print(f"seed {seed}: per-tensor {errs['per_tensor']:.3e}, per-channel {errs['per_channel']:.3e}, factor {errs['per_tensor'] / errs['per_channel']:.1f}")
    assert errs["per_channel"] <= errs["per_tensor"] / 10, errs


def test_record_the_reference_cnns_error_against_the_float_model():
    """recorded only: both chained twins of the reference CNN against the float model on inputs like the calibration set's"""
    import taper_amd as T
    rng = np.random.default_rng(81)
    model = B.get("hip").sequential(B.nonzero_biases(B.cnn_reference(rng), rng))
    shape = (16, 1, 28, 28)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    xt = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    fl = model.forward(xt).data()
    for name, twin in (("cnn_reference_per_tensor_vs_float", model.quantize_static_chain(calib)),
                       ("cnn_reference_per_channel_vs_float", model.quantize_static_per_channel(calib))):
        rec = margins.record("test_gpu_qperchan_accuracy", name, twin(xt).data(), fl)
        print(f"{name}: {rec['err_over_scale']:.3e} of max |y|")
    T.Tape.reset()
