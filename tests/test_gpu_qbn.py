"""A frozen BatchNorm2d in the quantized twins on the GPU: th_fold_batchnorm2d, th_channel_affine_fwd, the AFFINE form of the
int8 conv product in both output forms, and BatchNorm2d / BasicBlock models through every static quantize call, against the numpy restatement of
tests/qbn_ref.py.  The integer sums are exact and every f32 operation rounds once, so the comparisons with the restatement are on bits."""
import ctypes as C

import numpy as np
import pytest

from oracle import train_extra as OX
from tests import margins
from tests import qbn_ref as N
from tests import qconv_ref as Q
from tests import qperchan_ref as P
from tests import qstatic_ref as R
from tests import test_gpu_qchain as TCH
from tests import test_gpu_qconv as TC
from tests import test_gpu_qperchan as TP

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, GUARD_BITS, FILL = TC.GUARD, TC.GUARD_BITS, TCH.FILL
BPARAMS = TC.BPARAMS
_bits, _in_use, _lib, _pool_in_use = TC._bits, TC._in_use, TC._lib, TC._pool_in_use
CONVS, CHAIN, PER_CHANNEL = 1, 2, 4


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def int_affine(c):
    """goes with sx = 1 and integer weight pairs: a = +-(1 + i % 3), b = i % 5 - 2 -- every value an integer, a pair that reaches another channel shows"""
    i = np.arange(c)
    return np.stack([((1 + i % 3) * np.where(i % 2, -1, 1)).astype(f32), (i % 5 - 2).astype(f32)], axis=1)


def float_affine(c):
    """another pair in every channel: both signs of a, a zero a, and b of the size of the values"""
    i = np.arange(c, dtype=f32)
    a = ((f32(0.5) + f32(0.013) * i) * np.where(np.arange(c) % 3 == 1, f32(-1), f32(1))).astype(f32)
    if c > 2:
        a[2] = 0
    return np.stack([a, (f32(0.37) * (i % 7 - 3)).astype(f32)], axis=1)


# ---------------------------------------------------------------- 1: the fold
def _fold_call(ctx, gamma, beta, mean, var, eps):
    c = gamma.size
    out = ctx.upload(np.full(2 * c + 2 * GUARD, GUARD_BITS, np.uint32))
    before = _in_use(ctx)
    ctx.call("th_fold_batchnorm2d", ctx.upload(gamma), ctx.upload(beta), ctx.upload(mean), ctx.upload(var), float(eps), c, out.offset(4 * GUARD))
    assert _in_use(ctx) == before
    raw = ctx.download(out, (2 * c + 2 * GUARD,), np.uint32)
    assert (raw[:GUARD] == GUARD_BITS).all() and (raw[GUARD + 2 * c:] == GUARD_BITS).all(), "words around the pairs were written"
    return raw[GUARD:GUARD + 2 * c].view(f32).reshape(c, 2)


@pytest.mark.parametrize("c", [1, 5, 130])
def test_fold_is_the_reference_bit_for_bit(ctx, c):
    rng = np.random.default_rng(c)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32)
    beta, mean = (0.1 * rng.standard_normal(c)).astype(f32), rng.standard_normal(c).astype(f32)
    var = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), c)).astype(f32)
    if c >= 5:
        gamma[1], gamma[2], var[3], var[4], gamma[4] = 0.0, -0.75, 0.0, 0.0, -1.25      # a zero and a negative gamma, var == 0 (with both signs of gamma)
    else:
        gamma[0], var[0] = -0.75, 0.0
    for eps in (1e-5, 1e-3):
        ref = N.fold(gamma, beta, mean, var, eps)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(_bits(_fold_call(ctx, gamma, beta, mean, var, eps)), _bits(ref), err_msg=str((c, eps)))


# ---------------------------------------------------------------- 2: the standalone layer
def _affine_call(ctx, x, ab, relu, shift):
    """one th_channel_affine_fwd call; shift: both d_x and d_y one float past a 16-byte boundary (the scalar path)"""
    n, c, h, w = x.shape
    xbuf = ctx.upload(np.concatenate([np.zeros(4 + shift, f32), x.reshape(-1)]))
    ybuf = ctx.upload(np.full(x.size + 2 * GUARD + shift, GUARD_BITS, np.uint32))
    dab = ctx.upload(ab)
    before = _in_use(ctx)
    ctx.call("th_channel_affine_fwd", xbuf.offset(4 * (4 + shift)), dab, n, c, h * w, relu, ybuf.offset(4 * (GUARD + shift)))
    assert _in_use(ctx) == before
    raw = ctx.download(ybuf, (x.size + 2 * GUARD + shift,), np.uint32)
    lo = GUARD + shift
    assert (raw[:lo] == GUARD_BITS).all() and (raw[lo + x.size:] == GUARD_BITS).all(), "words around the output were written"
    return raw[lo:lo + x.size].view(f32).reshape(x.shape)


# hw % 4 != 0; hw == 1 over two channel tiles' worth of channels; the 16-byte path; several trips of a lane's walk, planes of 625 float4s
AFFINE_SHAPES = [(2, 5, 3, 3), (1, 130, 1, 1), (3, 4, 2, 2), (8, 130, 50, 50)]


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_standalone_affine_is_the_reference_bit_for_bit(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(f32)
    ab = float_affine(shape[1])
    for shift in (0, 1):      # (an aligned call of a shape with hw % 4 != 0 is scalar too)
        for relu in (0, 1):
            ref = N.affine(x, ab, relu)
            np.testing.assert_array_equal(_bits(_affine_call(ctx, x, ab, relu, shift)), _bits(ref), err_msg=str((shape, "shift", shift, "relu", relu)))
    assert (N.affine(x, ab, 1) == 0).any() and (N.affine(x, ab, 0) < 0).any()


# ---------------------------------------------------------------- 3: the products
C_IN, C_OUT = (1, 3, 17), (4, 33, 65, 128, 130)
MAPS = ((2, 7, 9), (1, 12, 12))      # n, h, w: 126 (or 70) pixels across two images; 144 (or 100): more than one pixel tile


def test_product_case_table_reaches_every_form_and_edge():
    plans = {co: TC.plan(2, 3, 7, 9, co, (3, 3), (1, 1), (1, 1)) for co in C_OUT}
    assert [plans[co]["nt"] for co in C_OUT] == [1, 2, 4, 4, 4]
    assert plans[130]["tiles_n"] == 2 and all(plans[co]["tiles_n"] == 1 for co in C_OUT[:4])
    assert plans[4]["tiles_m"] == 1 and 2 * 7 * 9 % plans[4]["tile_m"] != 0
    assert TC.plan(1, 3, 12, 12, 4, (3, 3), (1, 1), (1, 1))["tiles_m"] == 2


def _product_affine(ctx, qx, sx, qw, wparams, qb, bparams, pad, relu, ab, per_channel):
    """one th_conv2d_q8q8_fwd_affine call (3x3, stride 1), the output NaN-filled between guard words that must come back untouched"""
    n, c_in, h, w = qx.shape
    c_out = qw.shape[0]
    pitch = Q.cpitch(c_in)
    ho, wo = Q.out_hw(h, w, (3, 3), (1, 1), pad)
    total = n * c_out * ho * wo
    dx, dw = ctx.upload(Q.nhwc(qx, pitch).view(np.uint8)), ctx.upload(Q.pack_weight(qw, pitch, 0x55).view(np.uint8))
    dps, dsx, dwp = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32)), ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wparams, f32))
    db = ctx.upload(qb.view(np.uint8)) if qb is not None else None
    dbp = ctx.upload(np.array(bparams, f32)) if qb is not None else None
    dab = ctx.upload(np.asarray(ab, f32))
    ybuf = ctx.upload(np.full(total + 2 * GUARD, GUARD_BITS, np.uint32))
    y = ybuf.offset(4 * GUARD)
    ctx.call("th_fill_f32", y, float("nan"), total)
    before = _in_use(ctx)
    ctx.call("th_conv2d_q8q8_fwd_affine", dx, pitch, dps, dsx, n, c_in, h, w, dw, c_out, 3, 3, 1, 1, pad[0], pad[1], dwp, db, dbp, relu, y, per_channel, dab)
    assert _in_use(ctx) == before
    out = ctx.download(ybuf, (total + 2 * GUARD,), np.uint32)
    assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + total:] == GUARD_BITS).all(), "words around the output were written"
    return out[GUARD:GUARD + total].view(f32).reshape(n, c_out, ho, wo)


def _codes_affine(ctx, qx, sx, qw, wparams, qb, bparams, pad, relu, ab, per_channel, sy, pitch_y, want_sums):
    """one th_conv2d_q8q8_fwd_codes_affine call into buffers prefilled with 0x55 between guard regions that must come back untouched"""
    n, c_in, h, w = qx.shape
    c_out = qw.shape[0]
    pitch = Q.cpitch(c_in)
    ho, wo = Q.out_hw(h, w, (3, 3), (1, 1), pad)
    px = n * ho * wo
    dx, dw = ctx.upload(Q.nhwc(qx, pitch).view(np.uint8)), ctx.upload(Q.pack_weight(qw, pitch, 0x55).view(np.uint8))
    dps, dsx, dwp = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32)), ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wparams, f32))
    db = ctx.upload(qb.view(np.uint8)) if qb is not None else None
    dbp = ctx.upload(np.array(bparams, f32)) if qb is not None else None
    dab, dsy = ctx.upload(np.asarray(ab, f32)), ctx.upload(np.array([sy], f32))
    G = TCH.GUARD
    qbuf = ctx.upload(np.full(px * pitch_y + 2 * G, FILL, np.uint8))
    sbuf = ctx.upload(np.full(px + 2 * G, FILL, np.int32))
    before = _in_use(ctx)
    ctx.call("th_conv2d_q8q8_fwd_codes_affine", dx, pitch, dps, dsx, n, c_in, h, w, dw, c_out, 3, 3, 1, 1, pad[0], pad[1], dwp, db, dbp, relu, dsy,
             qbuf.offset(G), pitch_y, sbuf.offset(4 * G) if want_sums else None, per_channel, dab)
    assert _in_use(ctx) == before
    qraw, sraw = ctx.download(qbuf, (px * pitch_y + 2 * G,), np.uint8), ctx.download(sbuf, (px + 2 * G,), np.int32)
    assert (qraw[:G] == FILL).all() and (qraw[G + px * pitch_y:] == FILL).all(), "bytes around the codes were written"
    assert (sraw[:G] == FILL).all() and (sraw[G + px:] == FILL).all(), "words around the pixel sums were written"
    return qraw[G:G + px * pitch_y].view(np.int8).reshape(n, ho, wo, pitch_y), sraw[G:G + px].reshape(n, ho, wo)


def _pair_sets(c_out, per_channel):
    """(sx, weight pairs, affine): pure integers (they pin the lane maps), then floats"""
    if per_channel:
        return [(1.0, TP.int_pairs(c_out), int_affine(c_out)), (0.0173, TP.float_pairs(c_out), float_affine(c_out))]
    return [(TC.PARAMS[0][0], TC.PARAMS[0][1], int_affine(c_out)), (TC.PARAMS[1][0], TC.PARAMS[1][1], float_affine(c_out))]


@pytest.mark.parametrize("c_out", C_OUT)
@pytest.mark.parametrize("c_in", C_IN)
def test_affine_product_is_the_reference_bit_for_bit(ctx, c_in, c_out):
    calls = 0
    for n, h, w in MAPS:
        qx, qw, qb = TC._operands(n, c_in, h, w, c_out, (3, 3), seed=100 * c_in + c_out + h)
        for pad in ((0, 0), (1, 1)):
            for per_channel in (0, 1):
                for k, (sx, wp, ab) in enumerate(_pair_sets(c_out, per_channel)):
                    for bias, relu in TP.FORMS:
                        if k == 0 and (bias, relu) in ((0, 1), (1, 0)):      # the integer set pins the maps: two forms do
                            continue
                        ref = N.conv_q8q8_affine(qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), pad, relu, ab, per_channel)
                        got = _product_affine(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, pad, relu, ab, per_channel)
                        assert not np.isnan(ref).any()
                        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str(((n, h, w), pad, "pc", per_channel, sx, "bias", bias, "relu", relu)))
                        calls += 1
    assert calls == 2 * 2 * 2 * 6


@pytest.mark.parametrize("c_out", [c for c in C_OUT if c <= 128])
@pytest.mark.parametrize("c_in", C_IN)
def test_affine_codes_padding_and_pixel_sums_are_the_reference(ctx, c_in, c_out):
    tile = TC.plan(1, c_in, 12, 12, c_out, (3, 3), (1, 1), (1, 1))["tile_n"]
    case = 0
    for n, h, w in MAPS:
        qx, qw, qb = TC._operands(n, c_in, h, w, c_out, (3, 3), seed=200 * c_in + c_out + h)
        for pad in ((0, 0), (1, 1)):
            for per_channel in (0, 1):
                sx, wp, ab = _pair_sets(c_out, per_channel)[1]
                for bias, relu in TP.FORMS:
                    case += 1
                    want_sums, extra = case % 2, (0, 16, tile)[case % 3]      # the tightest pitch, a looser one, one beyond the channel tile
                    pitch_y = Q.cpitch(c_out) + extra
                    assert extra != tile or pitch_y > tile
                    y = N.conv_q8q8_affine(qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), pad, relu, ab, per_channel)
                    sy = f32(R.act_scale_of(y) * f32(0.6))      # the next layer's scale: the outer 40 % of the range saturates
                    ref_q, ref_ps = N.conv_q8q8_codes_affine(qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), pad, relu, ab, per_channel, sy, pitch_y)
                    got_q, got_ps = _codes_affine(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, pad, relu, ab, per_channel, sy, pitch_y, want_sums)
                    what = str(((n, h, w), pad, "pc", per_channel, "bias", bias, "relu", relu, "pitch", pitch_y))
                    np.testing.assert_array_equal(got_q[..., :c_out], ref_q[..., :c_out], err_msg=what)
                    assert not got_q[..., c_out:].any(), "padding bytes must be 0: " + what
                    if want_sums:
                        np.testing.assert_array_equal(got_ps, ref_ps, err_msg=what)
                    else:
                        assert (got_ps == FILL).all(), "pixel sums were written although none were asked for"
    assert case >= 32


@pytest.mark.parametrize("c_out", [33, 130])
def test_an_affine_of_ones_and_zeros_gives_the_pc_entrys_values(ctx, c_out):
    pc = TP._PerChannel(ctx)
    qx, qw, qb = TC._operands(2, 17, 7, 9, c_out, (3, 3), seed=c_out)
    sx, wp, _ = _pair_sets(c_out, 1)[1]
    for bias, relu in TP.FORMS:
        a = _product_affine(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), relu, N.identity(c_out), 1)
        b = TC._product(pc, qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), (1, 1), relu, Q.cpitch(17))
        assert np.array_equal(a, b), (c_out, bias, relu)      # as values: -0 + 0 is +0
        if c_out > 128:
            continue
        sy = f32(R.act_scale_of(b) * f32(0.6))
        qa, sa = _codes_affine(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), relu, N.identity(c_out), 1, sy, Q.cpitch(c_out), 1)
        qb_, sb = TCH._codes_call(pc, qx, sx, qw, wp, qb if bias else None, BPARAMS, (1, 1), (1, 1), relu, sy, Q.cpitch(c_out), True)
        np.testing.assert_array_equal(qa, qb_)
        np.testing.assert_array_equal(sa, sb)
    one = TC.PARAMS[1][1]      # per_channel == 0 reads one pair: the per-tensor entry's values
    a = _product_affine(ctx, qx, sx, qw, one, qb, BPARAMS, (1, 1), 1, N.identity(c_out), 0)
    assert np.array_equal(a, TC._product(ctx, qx, sx, qw, one, qb, BPARAMS, (1, 1), (1, 1), 1, Q.cpitch(17)))


# ---------------------------------------------------------------- 4: refusals
def test_refusals_name_the_function_launch_nothing_and_the_next_call_succeeds(ctx):
    hip = _lib()
    # the fold
    c = 5
    g, b, m, v = (ctx.upload(np.full(c, k, f32)) for k in (1.5, 0.25, 0.5, 4.0))
    out = ctx.upload(np.full(2 * c, GUARD_BITS, np.uint32))
    good = dict(g=int(g), b=int(b), m=int(m), v=int(v), eps=1e-5, c=c, out=int(out))

    def fold(**kw):
        a = dict(good, **kw)
        return hip.th_fold_batchnorm2d(ctx.h, a["g"], a["b"], a["m"], a["v"], a["eps"], a["c"], a["out"])

    before = _in_use(ctx)
    for what, kw in (("null gamma", dict(g=None)), ("null beta", dict(b=None)), ("null mean", dict(m=None)), ("null var", dict(v=None)), ("null out", dict(out=None)),
                     ("c 0", dict(c=0)), ("c negative", dict(c=-3)), ("eps 0", dict(eps=0.0)), ("eps negative", dict(eps=-1e-5)), ("eps nan", dict(eps=float("nan"))),
                     ("eps inf", dict(eps=float("inf")))):
        assert fold(**kw) != 0 and b"th_fold_batchnorm2d" in hip.th_last_error(), what
    assert hip.th_fold_batchnorm2d(None, good["g"], good["b"], good["m"], good["v"], 1e-5, c, good["out"]) != 0
    assert _in_use(ctx) == before
    assert (ctx.download(out, (2 * c,), np.uint32) == GUARD_BITS).all(), "a refused call wrote"
    assert fold() == 0
    np.testing.assert_array_equal(_bits(ctx.download(out, (c, 2))), _bits(N.fold(*(np.full(c, k, f32) for k in (1.5, 0.25, 0.5, 4.0)), 1e-5)))

    # the standalone layer
    x = np.random.default_rng(1).standard_normal((2, c, 2, 2)).astype(f32)
    dx, dy = ctx.upload(x), ctx.upload(np.full(x.size, GUARD_BITS, np.uint32))
    good = dict(x=int(dx), ab=int(out), n=2, c=c, hw=4, y=int(dy))

    def aff(**kw):
        a = dict(good, **kw)
        return hip.th_channel_affine_fwd(ctx.h, a["x"], a["ab"], a["n"], a["c"], a["hw"], 1, a["y"])

    before = _in_use(ctx)
    for what, kw in (("null x", dict(x=None)), ("null pairs", dict(ab=None)), ("null y", dict(y=None)), ("n negative", dict(n=-1)), ("c 0", dict(c=0)),
                     ("hw 0", dict(hw=0)), ("hw negative", dict(hw=-4)), ("2^31 elements a channel", dict(n=65536, hw=32768))):
        assert aff(**kw) != 0 and b"th_channel_affine_fwd" in hip.th_last_error(), what
    assert hip.th_channel_affine_fwd(None, good["x"], good["ab"], 2, c, 4, 1, good["y"]) != 0
    assert aff(n=0) == 0, "an empty batch is no error"
    assert _in_use(ctx) == before
    assert (ctx.download(dy, (x.size,), np.uint32) == GUARD_BITS).all(), "a refused or an empty call wrote"
    assert aff() == 0
    np.testing.assert_array_equal(_bits(ctx.download(dy, x.shape)), _bits(N.affine(x, ctx.download(out, (c, 2)), 1)))

    # the products: a null d_affine, and the twins' refusals under the new names
    n, c_in, h, w = 1, 16, 5, 5
    qx, qw, _ = TC._operands(n, c_in, h, w, 129, (3, 3), seed=5)
    dqx, dqw = ctx.upload(Q.nhwc(qx, 16).view(np.uint8)), ctx.upload(Q.pack_weight(qw, 16).view(np.uint8))
    dps = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32))
    dsx, dwp, dsy, dab = ctx.upload(np.array([1.0], f32)), ctx.upload(TP.int_pairs(129)), ctx.upload(np.array([90000.0], f32)), ctx.upload(int_affine(129))
    dq, dsum = ctx.upload(np.full(9 * 144 + 64, FILL, np.uint8)), ctx.upload(np.full(9, FILL, np.int32))
    dyf = ctx.upload(np.full(9 * 129, GUARD_BITS, np.uint32))

    def codes(co, cpy, ab=int(dab), wp=int(dwp)):
        return hip.th_conv2d_q8q8_fwd_codes_affine(ctx.h, int(dqx), 16, int(dps), int(dsx), n, c_in, h, w, int(dqw), co, 3, 3, 1, 1, 0, 0, wp, None, None, 0,
                                                   int(dsy), int(dq), cpy, int(dsum), 1, ab)

    def plain(co=129, ab=int(dab), cpitch=16, y=int(dyf), k=3):
        return hip.th_conv2d_q8q8_fwd_affine(ctx.h, int(dqx), cpitch, int(dps), int(dsx), n, c_in, h, w, int(dqw), co, k, k, 1, 1, 0, 0, int(dwp), None, None, 0, y,
                                             1, ab)

    before = _in_use(ctx)
    assert codes(128, 128, ab=None) != 0 and b"th_conv2d_q8q8_fwd_codes_affine" in hip.th_last_error() and b"null" in hip.th_last_error()
    assert codes(129, 144) != 0 and b"th_conv2d_q8q8_fwd_codes_affine" in hip.th_last_error() and b"129" in hip.th_last_error()
    assert codes(128, 128, wp=None) != 0 and codes(128, 120) != 0 and b"th_conv2d_q8q8_fwd_codes_affine" in hip.th_last_error()
    assert plain(ab=None) != 0 and b"th_conv2d_q8q8_fwd_affine" in hip.th_last_error() and b"null" in hip.th_last_error()
    for kw in (dict(cpitch=24), dict(y=None), dict(co=0), dict(k=6)):
        assert plain(**kw) != 0 and b"th_conv2d_q8q8_fwd_affine" in hip.th_last_error(), kw
    assert _in_use(ctx) == before
    assert (ctx.download(dq, (9 * 144 + 64,), np.uint8) == FILL).all() and (ctx.download(dyf, (9 * 129,), np.uint32) == GUARD_BITS).all(), "a refused call wrote"
    assert codes(128, 128) == 0 and plain() == 0      # the next calls succeed
    ref_q, ref_ps = N.conv_q8q8_codes_affine(qx, 1.0, qw[:128], TP.int_pairs(128), None, None, (1, 1), (0, 0), False, int_affine(128), 1, 90000.0, 128)
    np.testing.assert_array_equal(ctx.download(dq, (1, 3, 3, 128), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(dsum, (1, 3, 3), np.int32), ref_ps)
    ref = N.conv_q8q8_affine(qx, 1.0, qw, TP.int_pairs(129), None, None, (1, 1), (0, 0), False, int_affine(129), 1)
    np.testing.assert_array_equal(_bits(ctx.download(dyf, (1, 129, 3, 3))), _bits(ref))
    assert len(np.unique(ref_q)) > 8


# ---------------------------------------------------------------- 5: a BatchNorm model through every static quantize call
SHAPE = (16, 1, 12, 12)
FLAGS = (0, CONVS, CONVS | CHAIN, PER_CHANNEL, PER_CHANNEL | CONVS, PER_CHANNEL | CONVS | CHAIN)


def _set_bn(bn, rng):
    c = bn.num_features
    bn.gamma.set_data((rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32))
    bn.beta.set_data((0.1 * rng.standard_normal(c)).astype(f32))


def _bn_model(rng, shape=SHAPE):
    """the issue's model, its running statistics from three training-mode forwards; left in training mode"""
    import taper_amd as T
    bn1, bn2 = T.BatchNorm2d(8), T.BatchNorm2d(16, fuse_relu=True)
    layers = [T.Conv2d(1, 8, (3, 3), None, (1, 1)), bn1, T.ReLU(), T.MaxPool2d((2, 2), (2, 2)), T.Conv2d(8, 16, (3, 3), None, (1, 1)), bn2, T.Flatten(1),
              T.Linear(16 * 6 * 6, 10, True)]
    model = T.Sequential(layers)
    for l, k in ((layers[0], 9), (layers[4], 72), (layers[7], 576)):
        w, b = l.parameters()
        w.set_data((rng.standard_normal(w.numel()) / np.sqrt(k)).astype(f32))
        b.set_data((0.1 * rng.standard_normal(b.numel())).astype(f32))
    _set_bn(bn1, rng)
    _set_bn(bn2, rng)
    model.train()
    for _ in range(3):
        model.forward(T.Tensor(rng.standard_normal(shape).astype(f32), shape))
    T.Tape.reset()
    return model, layers


def _static_ex(model, calib, flags):
    import taper_amd as T
    from taper_amd._lib import host
    arr = (C.c_void_p * len(calib))(*[t._h for t in calib])
    h = C.c_void_p()
    assert host.tp_module_quantize_static_ex(model._h, arr, len(calib), flags, C.byref(h)) == 0, host.tp_last_error()
    return T.QuantizedModule(h.value)


def _state(model, bns):
    return ([_bits(p.data()).copy() for p in model.parameters()], [_bits(b.data()).copy() for b in model.buffers()], [bn.is_training() for bn in bns])


def _folds(bns):
    return [N.fold(bn.gamma.data(), bn.beta.data(), bn.running_mean, bn.running_var, 1e-5) for bn in bns]


def _deq(kind, codes, params):
    return OX.dequantize_int8(codes, params[1], -128, params[0]) if kind == "int8" else OX.f16_bits_to_f32(codes)


def _ref_static(ts, scales, abs_, x, pc):
    """the twin with static convs from its packed tensors, scales and pairs (max pool and flatten are exact in numpy)"""
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2), (_, w3, p3), (_, b3, q3) = ts
    h = N.conv_q8q8_affine(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 8, 1, (3, 3)), p1, b1, q1, (1, 1), (1, 1), True, abs_[0], pc)
    h = Q.max_pool(h, (2, 2), (2, 2))
    h = N.conv_q8q8_affine(Q.quantize_act_nchw(h, scales[1])[0], scales[1], Q.taper_weight(w2, 16, 8, (3, 3)), p2, b2, q2, (1, 1), (1, 1), True, abs_[1], pc)
    return (P.linear_q8q8_pc if pc else R.linear_q8q8)(R.quantize_act(h.reshape(x.shape[0], -1), scales[2])[0], scales[2], w3.reshape(10, 576), p3, b3, q3)


@pytest.fixture(scope="module")
def bn_twins():
    import taper_amd as T
    rng = np.random.default_rng(81)
    model, layers = _bn_model(rng)
    bns = [layers[1], layers[5]]
    calib = [T.Tensor(a, SHAPE) for a in (rng.standard_normal(SHAPE).astype(f32), (1.5 * rng.standard_normal(SHAPE)).astype(f32))]
    before = _state(model, bns)
    T.Tape.reset()
    twins = {f: _static_ex(model, calib, f) for f in FLAGS}
    tape_len = T.Tape.len()
    # the same layers without the BatchNorm2d ones (they share the parameters): what quantize("int8") packs of these weights
    plain8 = T.Sequential([l for l in layers if l not in bns]).quantize("int8").tensors()
    return dict(model=model, layers=layers, bns=bns, calib=calib, before=before, after=_state(model, bns), twins=twins, plain8=plain8, tape_len=tape_len)


def test_quantizing_reads_the_source_only(bn_twins):
    assert bn_twins["tape_len"] == 0
    b, a = bn_twins["before"], bn_twins["after"]
    assert b[2] == a[2] == [True, True], "the training flags moved"
    for x, y in zip(b[0] + b[1], a[0] + a[1]):
        np.testing.assert_array_equal(x, y)


def test_affines_scales_links_tensors_and_storage(bn_twins):
    model, twins, folds = bn_twins["model"], bn_twins["twins"], _folds(bn_twins["bns"])
    params = [p.data().reshape(-1) for p in model.parameters()]
    packed = [params[i] for i in (0, 1, 4, 5, 8, 9)]      # parameters() without BatchNorm's
    plain8 = bn_twins["plain8"]
    step = _lib().th_qlinear_i8_kstep()
    for name, q in twins.items():
        got = q.affines()
        assert [a.shape for a in got] == [(8, 2), (16, 2)] and all(a.dtype == f32 for a in got), name
        for a, ref in zip(got, folds):
            np.testing.assert_array_equal(_bits(a), _bits(ref), err_msg=str(name))
        ts = q.tensors()
        assert len(ts) == 6, name
        assert q.chain_links() == (1 if name & CHAIN else 0), name
        assert q.act_scales().shape == ((3,) if name & CONVS else (1,)), name
        for i, ((kind, codes, pairs), (_, c8, p8), v) in enumerate(zip(ts, plain8, packed)):
            assert kind == "int8"
            if isinstance(pairs, np.ndarray):      # a per-channel weight: the per-channel codec on the model's buffer
                assert name & PER_CHANNEL and i in (0, 2, 4)
                ref_q, ref_p = P.pack_channels(v.reshape(10, 576), 0) if i == 4 else P.taper_pack_channels(v, (8, 16)[i // 2], (1, 8)[i // 2], (3, 3))
                np.testing.assert_array_equal(codes, np.asarray(ref_q).reshape(-1), err_msg=str((name, i)))
                np.testing.assert_array_equal(_bits(pairs), _bits(ref_p))
            else:                                  # quantize("int8")'s bits
                ref_q, ref_p = R.pack(v)
                np.testing.assert_array_equal(codes, c8, err_msg=str((name, i)))
                np.testing.assert_array_equal(codes, ref_q.reshape(-1))
                np.testing.assert_array_equal(_bits(np.array(pairs, f32)), _bits(np.array(p8, f32)))
        n_pairs = sum(p.shape[0] if isinstance(p, np.ndarray) else 1 for _, _, p in ts)
        lin_pad = 10 * (-(-576 // step) * step) - 10 * 576
        share = sum(v.size for v in packed) + lin_pad + 8 * n_pairs + 4 * q.act_scales().size
        assert q.storage_bytes() == share + 8 * (8 + 16), name
    assert twins[PER_CHANNEL | CONVS].channel_layout(0) == (8, 1, 8) and twins[PER_CHANNEL].channel_layout(0) == (1, 0, 1)
    for f in (CONVS, CONVS | CHAIN, PER_CHANNEL | CONVS, PER_CHANNEL | CONVS | CHAIN):
        np.testing.assert_array_equal(_bits(twins[f].act_scales()), _bits(twins[CONVS].act_scales()))


def test_static_twins_are_the_reference_bit_for_bit_and_the_chain_changes_no_bit(bn_twins):
    import taper_amd as T
    twins, layers, calib = bn_twins["twins"], bn_twins["layers"], bn_twins["calib"]
    x = np.random.default_rng(82).standard_normal(SHAPE).astype(f32)
    far = (3 * 1.5 * 4 * np.sign(x)).astype(f32)          # beyond the calibration range: the first codes saturate
    far[:, :, :, ::3] = x[:, :, :, ::3]
    prefix = _static_ex(T.Sequential(layers[:7]), calib, 0)    # no Linear in it: the features of the twins whose convs stay weight-only
    feats = [prefix(T.Tensor(data, SHAPE)).data() for data in (x, far)]
    del prefix
    T.Tape.reset()
    before = _pool_in_use()
    for data, feat in zip((x, far), feats):
        out = {}
        for f, q in twins.items():
            y = q(T.Tensor(data, SHAPE).requires_grad())
            assert T.Tape.len() == 0 and y.tape_node() == 0
            out[f] = y.data()
            del y
            assert _pool_in_use() == before, f
            if f & CONVS:
                ref = _ref_static(q.tensors(), q.act_scales(), q.affines(), data, bool(f & PER_CHANNEL))
            else:
                (_, w, wp), (_, b, bp) = q.tensors()[4:]
                s = q.act_scales()[0]
                ref = (P.linear_q8q8_pc if f & PER_CHANNEL else R.linear_q8q8)(R.quantize_act(feat, s)[0], s, w.reshape(10, 576), wp, b, bp)
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0
            np.testing.assert_array_equal(_bits(out[f]), _bits(ref), err_msg=f"flags {f}")
        np.testing.assert_array_equal(_bits(out[CONVS]), _bits(out[CONVS | CHAIN]))
        np.testing.assert_array_equal(_bits(out[PER_CHANNEL | CONVS]), _bits(out[PER_CHANNEL | CONVS | CHAIN]))
        assert not np.array_equal(_bits(out[CONVS]), _bits(out[PER_CHANNEL | CONVS]))      # another codec: other bits
    q = twins[PER_CHANNEL | CONVS | CHAIN]
    got = q(T.Tensor(x, SHAPE)).data()
    for b in (0, 7, 15):
        alone = q(T.Tensor(x[b:b + 1], (1,) + SHAPE[1:])).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(got[b]), err_msg=f"image {b} alone")
    assert _pool_in_use() == before


def test_the_twin_is_a_snapshot_of_the_running_pair_whatever_the_flag_says():
    import taper_amd as T
    rng = np.random.default_rng(83)
    model, layers = _bn_model(rng)
    calib = [T.Tensor(rng.standard_normal(SHAPE).astype(f32), SHAPE)]
    x = T.Tensor(rng.standard_normal(SHAPE).astype(f32), SHAPE)
    a = _static_ex(model, calib, CONVS | CHAIN)
    ya = a(x).data()
    model.eval()
    b = _static_ex(model, calib, CONVS | CHAIN)
    assert [bn.is_training() for bn in (layers[1], layers[5])] == [False, False]
    np.testing.assert_array_equal(_bits(a.act_scales()), _bits(b.act_scales()))
    np.testing.assert_array_equal(_bits(ya), _bits(b(x).data()))
    model.train()
    model.forward(x)                                       # the source trains on: the running pair moves, the twin does not
    T.Tape.reset()
    assert not np.array_equal(_folds([layers[1]])[0], a.affines()[0])
    np.testing.assert_array_equal(_bits(ya), _bits(a(x).data()))


def test_weight_only_convs_inside_a_static_twin_follow_the_float_layers_on_the_dequantized_weights(bn_twins):
    """tests/test_gpu_quant.py's check and bound: the float kernels on the dequantized weights, with the restated affine in numpy.  Without
    CONVS both convs stay weight-only and both BatchNorm2d layers run th_channel_affine_fwd."""
    import taper_amd as T
    q = _static_ex(T.Sequential(bn_twins["layers"][:7]), bn_twins["calib"], 0)
    ts, abs_ = q.tensors(), q.affines()
    assert len(ts) == 4 and len(abs_) == 2 and q.act_scales().shape == (0,) and q.chain_links() == 0
    deq = [_deq(k, c, p) for k, c, p in ts]
    convs = [T.Conv2d(1, 8, (3, 3), None, (1, 1)), T.Conv2d(8, 16, (3, 3), None, (1, 1))]
    for cv, w, b in ((convs[0], deq[0], deq[1]), (convs[1], deq[2], deq[3])):
        cv.parameters()[0].set_data(w)
        cv.parameters()[1].set_data(b)
    x = np.random.default_rng(84).standard_normal(SHAPE).astype(f32)
    T.Tape.reset()
    y = q(T.Tensor(x, SHAPE).requires_grad())
    assert T.Tape.len() == 0 and y.tape_node() == 0
    h = N.affine(convs[0].forward(T.Tensor(x, SHAPE)).data(), abs_[0], True)
    h = Q.max_pool(h, (2, 2), (2, 2))
    ref = N.affine(convs[1].forward(T.Tensor(h, h.shape)).data(), abs_[1], True).reshape(16, -1)
    T.Tape.reset()
    err = float(np.abs(y.data().astype(np.float64) - ref).max() / max(1.0, float(np.abs(ref).max())))
    print(f"weight-only convs and standalone BatchNorm layers vs the float layers on the same weights: {err:.3e}")
    assert err <= 1e-4, err


def test_the_weight_only_quantize_keeps_the_reference_refusal():
    """quantize() is the reference's Module::quantize: BatchNorm2d and BasicBlock have no twin there (tests/test_gpu_batchnorm.py pins the
    message); they are deployed through the static calls"""
    import taper_amd as T
    models = [T.Sequential([T.BasicBlock(1, 4, seed=1), T.Flatten(1)]), T.Sequential([T.Conv2d(1, 4, (3, 3)), T.BatchNorm2d(4)]), T.BasicBlock(1, 4, seed=2)]
    T.Device.sync()
    before = _pool_in_use()
    for m in models:
        for kind in ("int8", "float16"):
            with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
                m.quantize(kind)
    assert _pool_in_use() == before


# ---------------------------------------------------------------- 6: blocks
def _set_block_stats(model, rng, shape):
    """running statistics from three training-mode forwards"""
    import taper_amd as T
    model.train()
    for _ in range(3):
        model.forward(T.Tensor(rng.standard_normal(shape).astype(f32), shape))
    T.Tape.reset()


def test_a_strided_block_stays_weight_only_and_its_batchnorm_runs_alone():
    import taper_amd as T
    rng = np.random.default_rng(91)
    shape = (4, 1, 8, 8)
    blocks = [T.BasicBlock(1, 8, 1, seed=3), T.BasicBlock(8, 8, 2, seed=4)]
    lin = T.Linear(8 * 4 * 4, 10, True, seed=5)
    model = T.Sequential(blocks + [T.Flatten(1), lin])
    for blk in blocks:      # parameters(): the conv's, then gamma, beta
        g, b = blk.parameters()[2:]
        g.set_data((rng.uniform(0.5, 1.5, 8) * rng.choice([-1.0, 1.0], 8)).astype(f32))
        b.set_data((0.1 * rng.standard_normal(8)).astype(f32))
    _set_block_stats(model, rng, shape)
    calib = [T.Tensor(rng.standard_normal(shape).astype(f32), shape)]
    T.Tape.reset()
    for flags in (CONVS | CHAIN, PER_CHANNEL | CONVS | CHAIN):
        pc = bool(flags & PER_CHANNEL)
        q = _static_ex(model, calib, flags)
        assert T.Tape.len() == 0
        ts, scales, abs_ = q.tensors(), q.act_scales(), q.affines()
        assert len(abs_) == 2 and scales.shape == (2,) and len(ts) == 6 and q.chain_links() == 0
        bufs = [b.data() for b in model.buffers()]
        for i, blk in enumerate(blocks):
            g, b = (p.data() for p in blk.parameters()[2:])
            np.testing.assert_array_equal(_bits(abs_[i]), _bits(N.fold(g, b, bufs[2 * i], bufs[2 * i + 1], 1e-5)))
        assert q.channel_layout(2) == (1, 0, 1) and q.channel_layout(0) == ((8, 1, 8) if pc else (1, 0, 1))      # the strided conv keeps one pair
        x = rng.standard_normal(shape).astype(f32)
        got = q(T.Tensor(x, shape)).data()
        (_, w1, p1), (_, b1, q1), (k2, w2, p2), (_, b2, q2), (_, w3, p3), (_, b3, q3) = ts
        h = N.conv_q8q8_affine(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 8, 1, (3, 3)), p1, b1, q1, (1, 1), (1, 1), True, abs_[0], pc)
        cv = T.Conv2d(8, 8, (3, 3), (2, 2), (1, 1))      # the float kernel the weight-only conv runs, on the dequantized weights
        cv.parameters()[0].set_data(_deq(k2, w2, p2))
        cv.parameters()[1].set_data(_deq(k2, b2, q2))
        h = N.affine(cv.forward(T.Tensor(h, h.shape)).data(), abs_[1], True)
        T.Tape.reset()
        assert h.shape == (4, 8, 4, 4)
        ref = (P.linear_q8q8_pc if pc else R.linear_q8q8)(R.quantize_act(h.reshape(4, -1), scales[1])[0], scales[1], w3.reshape(10, 128), p3, b3, q3)
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=f"flags {flags}")


def test_a_link_crosses_the_block_boundary_and_a_lone_block_is_a_pair():
    import taper_amd as T
    rng = np.random.default_rng(92)
    shape = (3, 1, 9, 7)
    blocks = [T.BasicBlock(1, 8, seed=6), T.BasicBlock(8, 16, seed=7)]
    model = T.Sequential(blocks)
    _set_block_stats(model, rng, shape)
    calib = [T.Tensor(rng.standard_normal(shape).astype(f32), shape)]
    x = rng.standard_normal(shape).astype(f32)
    for pcf in (0, PER_CHANNEL):
        chain, plain = _static_ex(model, calib, pcf | CONVS | CHAIN), _static_ex(model, calib, pcf | CONVS)
        assert chain.chain_links() == 1 and plain.chain_links() == 0
        assert chain.act_scales().shape == (2,) and len(chain.affines()) == 2 and len(chain.tensors()) == 4
        ts, scales, abs_ = chain.tensors(), chain.act_scales(), chain.affines()
        (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2) = ts
        h = N.conv_q8q8_affine(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 8, 1, (3, 3)), p1, b1, q1, (1, 1), (1, 1), True, abs_[0], bool(pcf))
        ref = N.conv_q8q8_affine(Q.quantize_act_nchw(h, scales[1])[0], scales[1], Q.taper_weight(w2, 16, 8, (3, 3)), p2, b2, q2, (1, 1), (1, 1), True, abs_[1], bool(pcf))
        got = chain(T.Tensor(x, shape)).data()
        np.testing.assert_array_equal(_bits(got), _bits(ref))
        np.testing.assert_array_equal(_bits(got), _bits(plain(T.Tensor(x, shape)).data()))
    lone = _static_ex(blocks[0], calib, CONVS | CHAIN)
    assert lone.act_scales().shape == (1,) and len(lone.affines()) == 1 and len(lone.tensors()) == 2 and lone.chain_links() == 0
    (_, w1, p1), (_, b1, q1) = lone.tensors()
    s = lone.act_scales()
    ref = N.conv_q8q8_affine(Q.quantize_act_nchw(x, s[0])[0], s[0], Q.taper_weight(w1, 8, 1, (3, 3)), p1, b1, q1, (1, 1), (1, 1), True, lone.affines()[0], False)
    np.testing.assert_array_equal(_bits(lone(T.Tensor(x, shape)).data()), _bits(ref))
    wo = _static_ex(blocks[0], calib, 0)      # nothing static in it: a weight-only conv and a standalone BatchNorm2d
    assert len(wo.affines()) == 1 and len(wo.tensors()) == 2 and wo.act_scales().shape == (0,)
    T.Tape.reset()


# ---------------------------------------------------------------- 7: the twins stand for the float model
def test_chained_twins_compute_the_float_models_function():
    """tests/test_gpu_qconv.py's structural bound and its argument: three int8 layers calibrated on inputs that include the test's stay
    within a few percent of max |y|, a wrong layout or a wrong fold (a pair of another channel, a sign, the mean left out) is off by the
    order of max |y| itself; 0.25 lies between and bounds no quantization noise.  The restatement alone, on the CPU over 8 seeds of this
    construction, gives 2.0e-2 to 3.3e-2; on an MI355X this seed gives 2.36e-2 (per-channel) and 2.48e-2 (per-tensor)."""
    import taper_amd as T
    rng = np.random.default_rng(95)
    model, _ = _bn_model(rng)
    x = rng.standard_normal(SHAPE).astype(f32)
    calib = [T.Tensor(a, SHAPE) for a in (rng.standard_normal(SHAPE).astype(f32), x)]
    twins = {"per_channel": _static_ex(model, calib, PER_CHANNEL | CONVS | CHAIN), "per_tensor": _static_ex(model, calib, CONVS | CHAIN)}
    model.eval()
    fl = model.forward(T.Tensor(x, SHAPE)).data()
    T.Tape.reset()
    for name, q in twins.items():
        assert q.chain_links() == 1
        got = q(T.Tensor(x, SHAPE)).data()
        rec = margins.record("test_gpu_qbn_stands_for_the_float_model", name, got, fl)
        err = float(np.abs(got - fl).max() / np.abs(fl).max())
        print(f"chained {name} twin vs the float model in eval mode: {err:.3e} of max |y| ({rec['err_over_scale']:.3e})")
        assert err <= 0.25, (name, err)


# ---------------------------------------------------------------- 8: every kind of step in one Sequential
ALL_SHAPE = (2, 2, 8, 8)


def _all_kinds_model(rng):
    """Every kind of step a Sequential twin resolves, the weight-only kind twice: a link through a folded BatchNorm2d, ReLU and pool; a
    grouped conv and a 1x1 conv that stay weight-only (two slots of one dequantize workspace); a BatchNorm2d that runs alone; a nested
    Sequential with a link inside and none across its boundary; a link across a BasicBlock's boundary; Linear + ReLU and a lone Linear."""
    import taper_amd as T
    pad = (1, 1)
    bns = [T.BatchNorm2d(4), T.BatchNorm2d(8)]
    model = T.Sequential([
        T.Conv2d(2, 4, (3, 3), None, pad, seed=11), bns[0], T.ReLU(), T.MaxPool2d((2, 2), (2, 2)), T.Conv2dReLU(4, 8, (3, 3), None, pad, seed=12),
        T.Conv2d(8, 8, (3, 3), None, pad, groups=2, seed=13), T.ReLU(),
        bns[1],
        T.Sequential([T.Conv2d(8, 4, (3, 3), None, pad, seed=14), T.Conv2d(4, 8, (3, 3), None, pad, seed=15)]),
        T.Conv2d(8, 4, (1, 1), seed=16),
        T.BasicBlock(4, 8, seed=17), T.Conv2d(8, 4, (3, 3), None, pad, seed=18),
        T.Flatten(1), T.Linear(4 * 4 * 4, 8, True, seed=19), T.ReLU(), T.Linear(8, 4, True, seed=20)])
    for bn in bns:
        _set_bn(bn, rng)
    _set_block_stats(model, rng, ALL_SHAPE)
    return model


def test_every_kind_of_step_in_one_sequential():
    """Chained and unchained twins of the model above agree on every output bit and on everything they report.  The links: conv ->
    BatchNorm2d -> ReLU -> pool -> Conv2dReLU, the two convs of the nested Sequential, the BasicBlock's conv -> the conv behind the block
    (3).  Static layers: 6 convs and 2 Linear; 8 convs and 2 Linear pack 20 tensors; 3 frozen BatchNorm2d."""
    import taper_amd as T
    rng = np.random.default_rng(97)
    model = _all_kinds_model(rng)
    calib = [T.Tensor(a, ALL_SHAPE) for a in (rng.standard_normal(ALL_SHAPE).astype(f32), (1.5 * rng.standard_normal(ALL_SHAPE)).astype(f32))]
    x = rng.standard_normal(ALL_SHAPE).astype(f32)
    far = (3 * 1.5 * 4 * np.sign(x)).astype(f32)          # beyond the calibration range: the first codes saturate
    far[:, :, :, ::3] = x[:, :, :, ::3]
    T.Tape.reset()

    def check(pcf):      # (a function: no twin of one pass is alive in the next, where the pool's occupancy is compared)
        chain, plain = _static_ex(model, calib, pcf | CONVS | CHAIN), _static_ex(model, calib, pcf | CONVS)
        assert chain.chain_links() == 3 and plain.chain_links() == 0
        assert chain.act_scales().shape == (8,)
        np.testing.assert_array_equal(_bits(chain.act_scales()), _bits(plain.act_scales()))
        assert chain.storage_bytes() == plain.storage_bytes()
        assert len(chain.affines()) == len(plain.affines()) == 3
        for a, b in zip(chain.affines(), plain.affines()):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        assert len(chain.tensors()) == len(plain.tensors()) == 20
        for i, ((ka, ca, pa), (kb, cb, pb)) in enumerate(zip(chain.tensors(), plain.tensors())):
            assert ka == kb and isinstance(pa, np.ndarray) == isinstance(pb, np.ndarray), i
            np.testing.assert_array_equal(ca, cb, err_msg=f"tensor {i}")
            np.testing.assert_array_equal(_bits(np.asarray(pa, f32)), _bits(np.asarray(pb, f32)), err_msg=f"tensor {i}")
        assert any(isinstance(p, np.ndarray) for _, _, p in chain.tensors()) == bool(pcf)
        before = _pool_in_use()
        for data in (x, far):
            outs = []
            for q in (chain, plain):
                y = q(T.Tensor(data, ALL_SHAPE))
                outs.append(y.data())
                del y
                assert _pool_in_use() == before
            assert outs[0].shape == (2, 4) and np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
            np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]), err_msg=f"flags {pcf}")
            for q, full in zip((chain, plain), outs):
                alone = q(T.Tensor(data[:1], (1,) + ALL_SHAPE[1:])).data()
                np.testing.assert_array_equal(_bits(alone[0]), _bits(full[0]), err_msg="image 0 alone")
                assert _pool_in_use() == before

    check(0)
    check(PER_CHANNEL)
