"""Calibrated int8 convolution on the GPU (csrc/qconv_i8.hip, Module.quantize_static_conv): the channel-last activation codec, the weight
re-layout, the implicit-GEMM product on the integer matrix cores and the static twin against the numpy restatement of tests/qconv_ref.py.
The accumulator is an exact int32 and the epilogue is four f32 operations rounded once each, so every comparison is on bits."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import qconv_ref as Q
from tests import qstatic_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
RTOL = 1e-4                # the scale of a layer behind float layers (tests/test_gpu_qstatic.py)
GUARD = 64                 # words on either side of an output
GUARD_BITS = 0xFFA5C3E1    # a NaN payload no computation produces
PARAMS = [(1.0, (0.0, 1.0)), (0.0173, (-0.31, 0.0024))]      # tests/test_gpu_qstatic.py's: pure integers (pins the lane maps), then a float codec
BPARAMS = (-0.27, 0.0019)


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


def _pool_in_use():
    import taper_amd as T
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- 1: the product alone, codes made on the host
# (n, c_in, h, w, c_out, (k_h, k_w), (s_h, s_w), (pad_h, pad_w)).  WHICH tile form a row takes and which edges it crosses is asserted
# through th_debug_qconv_plan (the host function the launch itself consumes) in tests/test_qconv_abi.py, not assumed.
PLAN_FIELDS = ("nt", "tile_m", "tile_n", "tiles_m", "tiles_n", "grid", "h_out", "w_out")


def plan(n, c_in, h, w, c_out, k, s, p):
    out = (C.c_int * 8)()
    assert _lib().th_debug_qconv_plan(n, c_in, h, w, c_out, k[0], k[1], s[0], s[1], p[0], p[1], C.cast(out, C.c_void_p)) == 0
    return dict(zip(PLAN_FIELDS, out))


CASES = [
    (1, 1, 15, 17, 1, (1, 1), (1, 1), (0, 0)),        # 255 pixels: one short of two pixel tiles; a single channel, a single input channel
    (2, 3, 8, 8, 31, (3, 3), (1, 1), (1, 1)),         # 128 pixels: exactly a tile, and it spans both images
    (5, 15, 7, 11, 32, (3, 3), (1, 1), (1, 1)),       # 385 pixels: one past three tiles; exactly a 32-channel tile
    (1, 16, 16, 16, 33, (3, 3), (1, 1), (1, 1)),      # 256 pixels: two whole tiles; the 64-channel form
    (3, 17, 9, 13, 63, (5, 5), (2, 2), (2, 2)),
    (2, 32, 12, 10, 64, (3, 2), (2, 1), (2, 1)),      # padding k - 1, stride (2, 1)
    (1, 64, 7, 7, 128, (3, 3), (1, 1), (1, 1)),       # the 128-channel form, exactly a tile
    (2, 16, 6, 5, 129, (3, 3), (1, 1), (0, 0)),       # one past it
    (1, 3, 8, 6, 127, (5, 5), (1, 1), (4, 4)),        # one short of it; padding k - 1: windows with a single in-image tap
    (1, 32, 4, 5, 260, (1, 1), (1, 1), (0, 0)),       # three channel tiles
    (4, 1, 12, 12, 4, (3, 3), (1, 1), (0, 0)),        # a first layer: 400 pixels, four tiles, every one across an image boundary or map rows
    (3, 64, 5, 7, 65, (3, 3), (2, 2), (1, 1)),
    (2, 17, 10, 7, 31, (5, 5), (2, 2), (2, 2)),
    (1, 15, 6, 9, 8, (3, 3), (1, 1), (2, 2)),
    (2, 16, 9, 9, 32, (1, 1), (2, 2), (0, 0)),
    (1, 3, 7, 5, 16, (3, 2), (1, 1), (1, 0)),
    (3, 32, 13, 16, 64, (3, 3), (1, 1), (1, 1)),      # 624 pixels by 64 channels: several pixel tiles in the 64-channel form
    (2, 16, 12, 11, 160, (3, 3), (1, 1), (1, 1)),     # 264 pixels by 160 channels: several tiles both ways in the 128-channel form
]
IDS = ["n{}-c{}-{}x{}-o{}-k{}x{}-s{}{}-p{}{}".format(c[0], c[1], c[2], c[3], c[4], *c[5], *c[6], *c[7]) for c in CASES]


def _operands(n, c_in, h, w, c_out, k, seed):
    """int8 codes over the full range from two different generators, -128 and 127 in both where there is room"""
    rng = np.random.default_rng(seed)
    qx = rng.integers(-128, 128, (n, c_in, h, w)).astype(np.int8)
    K = c_in * k[0] * k[1]
    o, j = np.meshgrid(np.arange(c_out), np.arange(K), indexing="ij")
    qw = ((o * 37 + j * 101 + (o * j) % 7 + rng.integers(0, 3, (c_out, K))) % 256 - 128).astype(np.int8).reshape(c_out, c_in, k[0], k[1])
    for q in (qx, qw):
        if q.size >= 2:
            q.reshape(-1)[0], q.reshape(-1)[-1] = -128, 127
    qb = rng.integers(-128, 128, c_out).astype(np.int8)
    return qx, qw, qb


def _product(ctx, qx, sx, qw, wparams, qb, bparams, stride, pad, relu, pitch):
    """one th_conv2d_q8q8_fwd call: x channel-last and zero padded, W's padding filled with a non-zero code (it must not matter), the
    output NaN-filled between two guard regions that must come back untouched, pool bytes in use unchanged"""
    n, c_in, h, w = qx.shape
    c_out, _, kh, kw = qw.shape
    ho, wo = Q.out_hw(h, w, (kh, kw), stride, pad)
    total = n * c_out * ho * wo
    pixsum = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    dx, dw = ctx.upload(Q.nhwc(qx, pitch).view(np.uint8)), ctx.upload(Q.pack_weight(qw, pitch, 0x55).view(np.uint8))
    dps, dsx, dwp = ctx.upload(pixsum), ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wparams, f32))
    db = ctx.upload(qb.view(np.uint8)) if qb is not None else None
    dbp = ctx.upload(np.array(bparams, f32)) if qb is not None else None
    ybuf = ctx.upload(np.full(total + 2 * GUARD, GUARD_BITS, np.uint32))
    y = ybuf.offset(4 * GUARD)
    ctx.call("th_fill_f32", y, float("nan"), total)
    before = _in_use(ctx)
    ctx.call("th_conv2d_q8q8_fwd", dx, pitch, dps, dsx, n, c_in, h, w, dw, c_out, kh, kw, stride[0], stride[1], pad[0], pad[1], dwp, db, dbp, relu, y)
    assert _in_use(ctx) == before
    out = ctx.download(ybuf, (total + 2 * GUARD,), np.uint32)
    assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + total:] == GUARD_BITS).all(), "words around the output were written"
    return out[GUARD:GUARD + total].view(f32).reshape(n, c_out, ho, wo)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product_is_the_reference_bit_for_bit(ctx, case):
    n, c_in, h, w, c_out, k, s, p = case
    i = CASES.index(case)
    qx, qw, qb = _operands(n, c_in, h, w, c_out, k, seed=1000 + i)
    pitch = Q.cpitch(c_in) + 16 * (i % 2)                      # the tightest pitch and a looser one
    for (sx, wp), (bias, relu) in zip(PARAMS + PARAMS, ((0, 0), (1, 0), (1, 1), (0, 1))):
        ref = Q.conv_q8q8(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu)
        got = _product(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, pitch)
        assert not np.isnan(ref).any()
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str((case, sx, wp, "bias", bias, "relu", relu)))


def test_product_at_the_largest_k_with_the_extreme_codes(ctx):
    """c_in = 4096, a 4 x 4 kernel on a 4 x 4 input: one output pixel at K = 65536, all -128 against all 127 (and the other corner)"""
    qx = np.full((1, 4096, 4, 4), -128, np.int8)
    qw = np.stack([np.full((4096, 4, 4), 127, np.int8), np.full((4096, 4, 4), -128, np.int8),
                   np.random.default_rng(1).integers(-128, 128, (4096, 4, 4)).astype(np.int8)])
    t, _ = R.int_terms(qx.reshape(1, -1), qw.reshape(3, -1))
    assert t.min() == -128 * 255 * R.MAX_K      # the largest |t| there is: inside int32
    for sx, wp in PARAMS:
        got = _product(ctx, qx, sx, qw, wp, None, None, (1, 1), (0, 0), 0, 4096)
        assert got.shape == (1, 3, 1, 1)
        np.testing.assert_array_equal(_bits(got), _bits(Q.conv_q8q8(qx, sx, qw, wp)))
    np.testing.assert_array_equal(_product(ctx, qx, 1.0, qw, (0.0, 1.0), None, None, (1, 1), (0, 0), 0, 4096).reshape(1, 3), t.astype(f32))


def test_an_images_result_does_not_depend_on_its_batch(ctx):
    case = (5, 15, 7, 11, 32, (3, 3), (1, 1), (1, 1))      # 77 pixels an image: every image starts at another place of a tile
    n, c_in, h, w, c_out, k, s, p = case
    qx, qw, qb = _operands(n, c_in, h, w, c_out, k, seed=77)
    sx, wp = PARAMS[1]
    whole = _product(ctx, qx, sx, qw, wp, qb, BPARAMS, s, p, 0, 16)
    for b in range(n):
        alone = _product(ctx, qx[b:b + 1], sx, qw, wp, qb, BPARAMS, s, p, 0, 16)
        np.testing.assert_array_equal(_bits(alone[0]), _bits(whole[b]), err_msg=f"image {b} alone")


# ---------------------------------------------------------------- 2: activations -> channel-last codes, weights -> channel-last codes
def _quantize_nhwc(ctx, x, dscale, pitch):
    n, c, h, w = x.shape
    nq, nps = n * h * w * pitch, n * h * w
    qbuf = ctx.upload(np.concatenate([np.full(4 * GUARD, 0xA5, np.uint8), np.full(nq, 0x55, np.uint8), np.full(4 * GUARD, 0xA5, np.uint8)]))
    pbuf = ctx.upload(np.full(nps + 2 * GUARD, GUARD_BITS, np.uint32))
    before = _in_use(ctx)
    ctx.call("th_quantize_act_nhwc_int8", ctx.upload(x), n, c, h, w, dscale, qbuf.offset(4 * GUARD), pitch, pbuf.offset(4 * GUARD))
    assert _in_use(ctx) == before
    qraw, praw = ctx.download(qbuf, (nq + 8 * GUARD,), np.uint8), ctx.download(pbuf, (nps + 2 * GUARD,), np.uint32)
    assert (qraw[:4 * GUARD] == 0xA5).all() and (qraw[4 * GUARD + nq:] == 0xA5).all(), "bytes around the codes were written"
    assert (praw[:GUARD] == GUARD_BITS).all() and (praw[GUARD + nps:] == GUARD_BITS).all(), "words around the pixel sums were written"
    return qraw[4 * GUARD:4 * GUARD + nq].view(np.int8).reshape(n, h, w, pitch), praw[GUARD:GUARD + nps].view(np.int32).reshape(n, h, w)


# c on both sides of a 16-byte piece and of a 64-channel turn; maps below, at and above a 64-pixel turn; odd maps
CODEC_SHAPES = [(1, 1, 5, 7), (2, 3, 5, 7), (3, 15, 3, 3), (1, 16, 8, 8), (2, 17, 9, 9), (3, 33, 5, 7), (2, 70, 9, 13), (1, 64, 1, 1)]


@pytest.mark.parametrize("shape", CODEC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_channel_last_codes_and_pixel_sums(ctx, shape):
    n, c, h, w = shape
    rng = np.random.default_rng(n * 1000 + c * 10 + h)
    x = (rng.standard_normal(shape) * 2).astype(f32)
    scale = R.act_scale_of(x)                                 # the scale is fixed beforehand: what follows lies outside it
    flat = x.reshape(-1)
    if flat.size >= 35:
        flat[3], flat[-1], flat[flat.size // 2] = np.nan, np.inf, -np.inf
        flat[7], flat[11] = 1e30, -1e30
    dscale = ctx.upload(np.array([scale], f32))
    ref_q, ref_ps = Q.quantize_act_nchw(x, scale)
    for pitch in (Q.cpitch(c), Q.cpitch(c) + 32):
        q, ps = _quantize_nhwc(ctx, x, dscale, pitch)
        np.testing.assert_array_equal(q[..., :c], ref_q.transpose(0, 2, 3, 1))
        assert not q[..., c:].any(), "padding bytes must be 0"
        np.testing.assert_array_equal(ps, ref_ps)
    if flat.size >= 35:
        r = ref_q.reshape(-1)
        assert r[3] == 0 and r[-1] == 127 and r[flat.size // 2] == -128 and r[7] == 127 and r[11] == -128
    assert _lib().th_qconv_i8_cpitch(c) == Q.cpitch(c)


def test_weight_pack_is_a_transpose_and_pad(ctx):
    rng = np.random.default_rng(2)
    for co, ci, kh, kw, pitch in ((1, 1, 1, 1, 16), (4, 1, 3, 3, 16), (5, 17, 3, 2, 32), (33, 16, 5, 5, 16), (8, 70, 3, 3, 96), (5, 33, 1, 1, 96)):
        src = rng.integers(-128, 128, (co, ci, kh, kw)).astype(np.int8)
        n = co * kh * kw * pitch
        dst = ctx.upload(np.concatenate([np.full(64, 0xA5, np.uint8), np.full(n, 0x7F, np.uint8), np.full(64, 0xA5, np.uint8)]))
        ctx.call("th_pack_conv_weight_int8", ctx.upload(src.view(np.uint8)), co, ci, kh, kw, dst.offset(64), pitch)
        raw = ctx.download(dst, (n + 128,), np.uint8)
        assert (raw[:64] == 0xA5).all() and (raw[64 + n:] == 0xA5).all()
        np.testing.assert_array_equal(raw[64:64 + n].view(np.int8).reshape(co, kh * kw, pitch), Q.pack_weight(src, pitch))
        if (kh, kw) == (1, 1):      # one tap: the rows of a Linear's weight, th_pad_rows_int8's (rows, k, pitch) -- the same bytes from either entry point
            rows = ctx.upload(np.full(n, 0x7F, np.uint8))
            ctx.call("th_pad_rows_int8", ctx.upload(src.view(np.uint8)), co, ci, rows, pitch)
            np.testing.assert_array_equal(ctx.download(rows, (n,), np.uint8), raw[64:64 + n])
        # the same buffer as a model's Conv2d reads it (weight_layout 0)
        ctx.call("th_pack_conv_weight_taper_int8", ctx.upload(src.view(np.uint8)), co, ci, kh, kw, dst.offset(64), pitch)
        raw = ctx.download(dst, (n + 128,), np.uint8)
        assert (raw[:64] == 0xA5).all() and (raw[64 + n:] == 0xA5).all()
        np.testing.assert_array_equal(raw[64:64 + n].view(np.int8).reshape(co, kh * kw, pitch), Q.pack_weight(Q.taper_weight(src, co, ci, (kh, kw)), pitch))


# ---------------------------------------------------------------- 3: refusals (host checks before any launch)
def test_refusals_name_the_function_and_the_next_call_succeeds(ctx):
    hip = _lib()
    n, c_in, h, w, c_out, k = 2, 16, 5, 5, 5, (3, 3)
    qx, qw, _ = _operands(n, c_in, h, w, c_out, k, seed=3)
    dx, dw = ctx.upload(Q.nhwc(qx, 32).view(np.uint8)), ctx.upload(Q.pack_weight(qw, 32).view(np.uint8))      # (room for the calls that must be refused)
    dps = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32))
    dsx, dwp, dy = ctx.upload(np.array([1.0], f32)), ctx.upload(np.array([0.0, 1.0], f32)), ctx.empty(n * c_out * 9)
    good = dict(x=int(dx), cp=32, ps=int(dps), sx=int(dsx), n=n, c=c_in, h=h, w=w, qw=int(dw), co=c_out, kh=3, kw=3, sh=1, sw=1, ph=0, pw=0, wp=int(dwp),
                qb=None, bp=None, y=int(dy))

    def call(**kw):
        a = dict(good, **kw)
        return hip.th_conv2d_q8q8_fwd(ctx.h, a["x"], a["cp"], a["ps"], a["sx"], a["n"], a["c"], a["h"], a["w"], a["qw"], a["co"], a["kh"], a["kw"], a["sh"],
                                      a["sw"], a["ph"], a["pw"], a["wp"], a["qb"], a["bp"], 0, a["y"])

    before = _in_use(ctx)
    for what, kw in (("null codes", dict(x=None)), ("null pixel sums", dict(ps=None)), ("null scale", dict(sx=None)), ("null weights", dict(qw=None)),
                     ("null weight params", dict(wp=None)), ("null output", dict(y=None)), ("a bias without its params", dict(qb=int(dw))),
                     ("x off 16 bytes", dict(x=int(dx) + 4)), ("w off 16 bytes", dict(qw=int(dw) + 8)), ("cpitch % 16", dict(cp=24)),
                     ("cpitch below c_in", dict(c=33)), ("n < 0", dict(n=-1)), ("c_in 0", dict(c=0)), ("h 0", dict(h=0)), ("c_out 0", dict(co=0)),
                     ("k_w 0", dict(kw=0)), ("stride 0", dict(sh=0)), ("negative padding", dict(pw=-1)), ("an empty output map", dict(kh=6)),
                     ("c_in k_h k_w above 65536", dict(c=4097, cp=4112, kh=4, kw=4, h=4, w=4))):
        assert call(**kw) != 0 and b"th_conv2d_q8q8_fwd" in hip.th_last_error(), what
    assert hip.th_conv2d_q8q8_fwd(None, *[good[f] for f in ("x", "cp", "ps", "sx", "n", "c", "h", "w", "qw", "co", "kh", "kw", "sh", "sw", "ph", "pw", "wp",
                                                              "qb", "bp")], 0, good["y"]) != 0
    assert hip.th_quantize_act_nhwc_int8(ctx.h, int(dy), 1, 8, 2, 2, int(dsx), int(dx), 24, int(dps)) != 0 and b"th_quantize_act_nhwc_int8" in hip.th_last_error()
    assert hip.th_quantize_act_nhwc_int8(ctx.h, int(dy), 1, 8, 2, 2, int(dsx), int(dx) + 4, 16, int(dps)) != 0 and b"th_quantize_act_nhwc_int8" in hip.th_last_error()
    assert hip.th_quantize_act_nhwc_int8(ctx.h, None, 1, 8, 2, 2, int(dsx), int(dx), 16, int(dps)) != 0 and b"th_quantize_act_nhwc_int8" in hip.th_last_error()
    assert hip.th_pack_conv_weight_int8(ctx.h, int(dx), 1, 8, 1, 1, int(dw), 24) != 0 and b"th_pack_conv_weight_int8" in hip.th_last_error()
    assert hip.th_pack_conv_weight_int8(ctx.h, int(dx), 1, 8, 1, 1, int(dw) + 4, 16) != 0 and b"th_pack_conv_weight_int8" in hip.th_last_error()
    assert hip.th_pack_conv_weight_taper_int8(ctx.h, int(dx), 1, 8, 1, 1, int(dw), 24) != 0 and b"th_pack_conv_weight_taper_int8" in hip.th_last_error()
    assert hip.th_pack_conv_weight_taper_int8(ctx.h, None, 1, 8, 1, 1, int(dw), 16) != 0 and b"th_pack_conv_weight_taper_int8" in hip.th_last_error()
    assert _in_use(ctx) == before
    assert call(n=0) == 0                                       # an empty batch is a shape: nothing is launched
    assert call() == 0
    np.testing.assert_array_equal(ctx.download(dy, (n, c_out, 3, 3)), Q.conv_q8q8(qx, 1.0, qw, (0.0, 1.0)))


# ---------------------------------------------------------------- 4: the twin of a small CNN
SHAPE = (8, 1, 12, 12)


def _cnn(rng):
    import taper_amd as T
    layers = [T.Conv2dReLU(1, 4, (3, 3)), T.MaxPool2d((2, 2), (2, 2)), T.Conv2d(4, 8, (3, 3), None, (1, 1)), T.ReLU(), T.MaxPool2d((2, 2), (2, 2)),
              T.Flatten(1), T.Linear(8 * 2 * 2, 10, True)]
    model = T.Sequential(layers)
    vals = [(0.4 * rng.standard_normal(p.numel())).astype(f32) for p in model.parameters()]
    for p, v in zip(model.parameters(), vals):
        p.set_data(v)
    return model, layers, vals


def _ref_chain(ts, scales, x):
    """the reference forward of the CNN from the twin's packed tensors and activation scales (max pool and flatten are exact in numpy).
    A conv's packed buffer holds its filters as the model's float conv reads them: Q.taper_weight."""
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2), (_, w3, p3), (_, b3, q3) = ts
    h = Q.conv_q8q8(Q.quantize_act_nchw(x, scales[0])[0], scales[0], Q.taper_weight(w1, 4, 1, (3, 3)), p1, b1, q1, relu=True)
    h = Q.max_pool(h, (2, 2), (2, 2))
    h = Q.conv_q8q8(Q.quantize_act_nchw(h, scales[1])[0], scales[1], Q.taper_weight(w2, 8, 4, (3, 3)), p2, b2, q2, pad=(1, 1), relu=True)
    h = Q.max_pool(h, (2, 2), (2, 2)).reshape(x.shape[0], -1)
    return R.linear_q8q8(R.quantize_act(h, scales[2])[0], scales[2], w3.reshape(10, 32), p3, b3, q3)


@pytest.fixture(scope="module")
def cnn_twin():
    import taper_amd as T
    rng = np.random.default_rng(51)
    model, layers, vals = _cnn(rng)
    calib = [rng.uniform(0, 1, SHAPE).astype(f32), (1.5 * rng.standard_normal(SHAPE)).astype(f32)]
    T.Tape.reset()
    q = model.quantize_static_conv([T.Tensor(c, SHAPE) for c in calib])
    return dict(model=model, layers=layers, vals=vals, calib=calib, q=q, tape_len=T.Tape.len(), ts=q.tensors(), scales=q.act_scales())


def test_twin_reports_a_scale_per_static_layer(cnn_twin):
    import taper_amd as T
    layers, calib, scales = cnn_twin["layers"], cnn_twin["calib"], cnn_twin["scales"]
    assert scales.dtype == f32 and scales.shape == (3,)
    assert _bits(scales[0]) == _bits(R.act_scale_of(*calib))      # the input's range is exact: min / max of the data
    for i, upto in ((1, 2), (2, 6)):                               # the second conv's input, the Linear's input
        prefix = T.Sequential(layers[:upto])
        ref = R.act_scale_of(*[prefix.forward(T.Tensor(c, SHAPE)).data() for c in calib])
        assert abs(float(scales[i]) - float(ref)) <= RTOL * float(ref), (i, scales[i], ref)
    assert cnn_twin["model"].quantize_static(T.Tensor(calib[0], SHAPE)).act_scales().shape == (1,)      # the old entry point: convs weight-only


def test_twin_packs_what_the_weight_only_twin_packs_and_reads_only(cnn_twin):
    m, vals, ts = cnn_twin["model"], cnn_twin["vals"], cnn_twin["ts"]
    assert cnn_twin["tape_len"] == 0
    for p, v in zip(m.parameters(), vals):
        np.testing.assert_array_equal(_bits(p.data()).reshape(-1), _bits(v))
    wo = m.quantize("int8").tensors()
    assert len(ts) == len(wo) == 6
    for (k1, c1, p1), (k2, c2, p2) in zip(ts, wo):
        assert k1 == k2 == "int8"
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))


def test_twin_forward_is_the_reference_chain_bit_for_bit(cnn_twin):
    import taper_amd as T
    q, ts, scales = cnn_twin["q"], cnn_twin["ts"], cnn_twin["scales"]
    x = np.random.default_rng(52).standard_normal(SHAPE).astype(f32)
    T.Tape.reset()
    xt = T.Tensor(x, SHAPE).requires_grad()
    before = _pool_in_use()
    y = q(xt)
    assert T.Tape.len() == 0 and y.tape_node() == 0
    got = y.data()
    del y
    assert _pool_in_use() == before      # codes, pixel sums and every intermediate map went back to the pool
    np.testing.assert_array_equal(_bits(got), _bits(_ref_chain(ts, scales, x)))
    for b in (0, 3, 7):
        alone = q(T.Tensor(x[b:b + 1], (1,) + SHAPE[1:])).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(got[b]), err_msg=f"image {b} alone")
    # three times beyond the calibration range: the codes saturate, as the reference's do
    far = (3 * max(np.abs(c).max() for c in cnn_twin["calib"]) * np.sign(x)).astype(f32)
    far[:, :, :, ::3] = x[:, :, :, ::3]
    assert np.abs(Q.quantize_act_nchw(far, scales[0])[0].astype(int)).max() == 128
    np.testing.assert_array_equal(_bits(q(T.Tensor(far, SHAPE)).data()), _bits(_ref_chain(ts, scales, far)))
    assert _pool_in_use() == before


# ---------------------------------------------------------------- 5: fallbacks and unchanged behaviour
def test_a_grouped_conv_stays_weight_only_inside_the_twin():
    import taper_amd as T
    rng = np.random.default_rng(61)
    front = [T.Conv2d(4, 8, (3, 3), None, (1, 1), None, 2), T.ReLU(), T.Flatten(1)]
    lin = T.Linear(8 * 6 * 6, 10, True)
    for p in front[0].parameters() + lin.parameters():
        p.set_data((0.3 * rng.standard_normal(p.numel())).astype(f32))
    model, prefix = T.Sequential(front + [lin]), T.Sequential(front)
    shape = (3, 4, 6, 6)
    imgs, calib = rng.standard_normal(shape).astype(f32), T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    q = model.quantize_static_conv(calib)
    scales, ts = q.act_scales(), q.tensors()
    assert scales.shape == (1,) and len(ts) == 4      # the Linear's scale alone: the grouped conv has no entry
    feat = prefix.quantize("int8").forward(T.Tensor(imgs, shape)).data()      # the weight-only twin of the same prefix
    (_, w, wp), (_, b, bp) = ts[2:]
    ref = R.linear_q8q8(R.quantize_act(feat, scales[0])[0], scales[0], w.reshape(10, 288), wp, b, bp)
    np.testing.assert_array_equal(_bits(q(T.Tensor(imgs, shape)).data()), _bits(ref))
    np.testing.assert_array_equal(_bits(q(T.Tensor(imgs, shape)).data()), _bits(model.quantize_static(calib)(T.Tensor(imgs, shape)).data()))


def test_convs_whose_float_path_is_no_plain_convolution_stay_weight_only():
    """a 5 x 5 stride-2 conv and a 1 x 1 conv: the float kernels behind them keep the reference's gathers (tensor.rs:1799-1801, 1931), so
    the twin keeps them on those kernels -- same bits as quantize_static's twin, no scale entry"""
    import taper_amd as T
    rng = np.random.default_rng(65)
    layers = [T.Conv2dReLU(2, 6, (5, 5), (2, 2), (2, 2)), T.Conv2d(6, 4, (1, 1)), T.Conv2dReLU(4, 4, (3, 3), None, (1, 1)), T.Flatten(1),
              T.Linear(4 * 5 * 5, 10, True)]
    model = T.Sequential(layers)
    for p in model.parameters():
        p.set_data((0.3 * rng.standard_normal(p.numel())).astype(f32))
    shape = (3, 2, 9, 9)
    calib, x = T.Tensor(rng.standard_normal(shape).astype(f32), shape), T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    q, old = model.quantize_static_conv(calib), model.quantize_static(calib)
    assert q.act_scales().shape == (2,) and old.act_scales().shape == (1,)      # the 3 x 3 conv and the Linear; the Linear alone
    front = T.Sequential(layers[:2])
    np.testing.assert_array_equal(_bits(T.Sequential(layers[:2]).quantize_static_conv(calib)(x).data()), _bits(front.quantize("int8")(x).data()))
    assert T.Sequential(layers[:2]).quantize_static_conv(calib).act_scales().shape == (0,)
    assert q(x).data().shape == (3, 10)


def test_on_a_linear_only_model_it_is_quantize_static():
    import taper_amd as T
    rng = np.random.default_rng(62)
    model = T.Sequential([T.Linear(100, 40, True, seed=5), T.ReLU(), T.Linear(40, 10, True, seed=6)])
    calib = [T.Tensor(rng.standard_normal((16, 100)).astype(f32), (16, 100)) for _ in range(2)]
    a, b = model.quantize_static_conv(calib), model.quantize_static(calib)
    np.testing.assert_array_equal(_bits(a.act_scales()), _bits(b.act_scales()))
    assert a.act_scales().shape == (2,) and a.storage_bytes() == b.storage_bytes()
    for (_, c1, p1), (_, c2, p2) in zip(a.tensors(), b.tensors()):
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))
    x = T.Tensor(rng.standard_normal((37, 100)).astype(f32), (37, 100))
    np.testing.assert_array_equal(_bits(a(x).data()), _bits(b(x).data()))


def test_qat_convs_calibrate_and_deploy_as_their_inner_layers():
    import taper_amd as T
    rng = np.random.default_rng(63)
    shape = (4, 3, 8, 8)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    plain = T.Sequential([T.Conv2dReLU(3, 8, (3, 3), None, (1, 1), seed=3), T.Flatten(1), T.Linear(8 * 64, 10, True, seed=4)])
    qat_model = T.Sequential([T.QATConv2d(3, 8, (3, 3), None, (1, 1), relu=True, seed=3), T.Flatten(1), T.QATLinear(8 * 64, 10, True, seed=4)])
    for a, b in zip(plain.parameters(), qat_model.parameters()):
        np.testing.assert_array_equal(_bits(a.data()), _bits(b.data()))
    ref = plain.quantize_static_conv(calib)
    T.qat.enable()
    try:
        T.Tape.reset()
        q = qat_model.quantize_static_conv(calib)
        assert T.Tape.len() == 0
    finally:
        T.qat.disable()
    assert q.act_scales().shape == (2,)
    np.testing.assert_array_equal(_bits(q.act_scales()), _bits(ref.act_scales()))
    for (_, c1, p1), (_, c2, p2) in zip(q.tensors(), ref.tensors()):
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    np.testing.assert_array_equal(_bits(q(x).data()), _bits(ref(x).data()))


def test_static_conv_refusals_leak_nothing():
    import taper_amd as T
    shape = (2, 1, 12, 12)
    x = T.Tensor(np.zeros(shape, f32), shape)
    model, _, _ = _cnn(np.random.default_rng(64))
    dropout = T.Sequential([T.Conv2d(1, 4, (3, 3)), T.Dropout(0.5)])
    wide = T.Sequential([T.Conv2d(7282, 1, (3, 3), bias=False)])      # 7282 * 9 = 65538
    T.Device.sync()
    before = _pool_in_use()
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static_conv(x)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        model.quantize_static_conv([])
    with pytest.raises(T.TaperError, match="undefined calibration tensor"):
        model.quantize_static_conv([x, None])
    with pytest.raises(T.TaperError, match="65538"):
        wide.quantize_static_conv(T.Tensor(np.zeros((1, 7282, 3, 3), f32), (1, 7282, 3, 3)))
    assert _pool_in_use() == before
    assert model.quantize_static_conv(x).act_scales().shape == (3,)      # and the next valid call succeeds


# ---------------------------------------------------------------- 6: the twin stands for the float model; accuracy beyond that is recorded only
def test_twin_computes_the_float_models_function():
    """Ties the twin to the float model, not to the restatement (which reads the weight layout as the code does).  The bound separates two
    orders of magnitude and bounds no quantization noise: an int8 code is off by at most 1 / 254 of its tensor's range (rms 0.23 %), so
    three int8 layers and their weight codes, calibrated on inputs like the test's, stay within a few percent of max |y|; filters read in
    another order give outputs unrelated to the model's, off by the order of max |y| itself.  0.25 lies between."""
    import taper_amd as T
    rng = np.random.default_rng(72)
    model, _, _ = _cnn(rng)
    shape = (64,) + SHAPE[1:]
    q = model.quantize_static_conv(T.Tensor(rng.standard_normal(shape).astype(f32), shape))
    xt = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    got, fl = q(xt).data(), model.forward(xt).data()
    T.Tape.reset()
    err = float(np.abs(got - fl).max() / np.abs(fl).max())
    print(f"static conv twin vs float model, matched calibration: {err:.3e} of max |y|")
    assert err <= 0.25, err


# ---------------------------------------------------------------- 7: accuracy, recorded only
def test_record_accuracy_against_the_float_model_and_the_weight_only_twin(cnn_twin):
    import taper_amd as T
    m, q = cnn_twin["model"], cnn_twin["q"]
    x = np.random.default_rng(71).standard_normal((64,) + SHAPE[1:]).astype(f32)
    xt = T.Tensor(x, x.shape)
    got, fl, wo = q(xt).data(), m.forward(xt).data(), m.quantize("int8")(xt).data()
    T.Tape.reset()
    for name, a, ref in (("static_conv_vs_float", got, fl), ("static_conv_vs_weight_only", got, wo)):
        rec = margins.record("test_gpu_qconv_accuracy", name, a, ref)
        print(f"{name}: {rec['err_over_scale']:.3e} of max |y|")
