"""Activations that stay int8 between static convolutions, on the GPU (csrc/qconv_i8.hip, Module.quantize_static_chain): the
product that writes the next layer's codes and the max-pool on codes against the numpy restatements of tests/qchain_ref.py, and the chained
twin against the unchained one (Module.quantize_static_conv).  Everything is an integer or an f32 operation rounded once, and a maximum
commutes with the monotone codec, so every comparison is on bits."""

import numpy as np
import pytest

from tests import backends as B
from tests import qchain_ref as QC
from tests import qconv_ref as Q
from tests import qstatic_ref as R
from tests.test_gpu_qconv import BPARAMS, PARAMS, _bits, _in_use, _lib, _operands, _pool_in_use, plan

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 256                # bytes on either side of the codes, words on either side of the pixel sums
FILL = 0x55                # what the output buffers hold before a call: a pooled buffer's garbage


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


# ---------------------------------------------------------------- 1: the product that writes codes
# (n, c_in, h, w, c_out, (k_h, k_w), (s_h, s_w), (pad_h, pad_w))
CASES = [
    (2, 3, 8, 8, 31, (3, 3), (1, 1), (1, 1)),         # a word cut by c_out; 128 pixels: one tile that spans both images
    (5, 15, 7, 11, 32, (3, 3), (1, 1), (1, 1)),       # 385 pixels: one past three tiles
    (1, 16, 16, 16, 33, (3, 3), (1, 1), (1, 1)),      # the 64-channel form with 15 padding bytes
    (1, 64, 7, 7, 128, (3, 3), (1, 1), (1, 1)),       # exactly the limit
    (1, 3, 8, 6, 127, (5, 5), (1, 1), (4, 4)),
    (3, 17, 9, 13, 63, (5, 5), (2, 2), (2, 2)),
    (4, 1, 12, 12, 4, (3, 3), (1, 1), (0, 0)),        # a first layer
    (1, 1, 15, 17, 1, (1, 1), (1, 1), (0, 0)),
]
IDS = ["n{}-c{}-{}x{}-o{}-k{}x{}-s{}{}-p{}{}".format(c[0], c[1], c[2], c[3], c[4], *c[5], *c[6], *c[7]) for c in CASES]


def assert_case_table_coverage():
    """through th_debug_qconv_plan, the host function the launch consumes (no GPU needed: tests/test_qchain_abi.py runs it too)"""
    rows = [(c, plan(*c)) for c in CASES]
    assert {p["nt"] for _, p in rows} == {1, 2, 4}
    assert all(p["tiles_n"] == 1 for _, p in rows)
    assert any(p["tiles_m"] > 1 for _, p in rows) and any(c[0] * p["h_out"] * p["w_out"] % p["tile_m"] == 1 for c, p in rows)
    assert any(c[4] % 4 for c, _ in rows) and any(c[4] == 128 for c, _ in rows) and any(Q.cpitch(c[4]) - c[4] == 15 for c, _ in rows)
    assert any(Q.cpitch(c[4]) < p["tile_n"] for c, p in rows), "a pitch below the channel tile: whole 16-byte pieces that are not stored"


def _codes_call(ctx, qx, sx, qw, wparams, qb, bparams, stride, pad, relu, sy, pitch_y, want_sums):
    """one th_conv2d_q8q8_fwd_codes call into buffers prefilled with 0x55 between guard regions that must come back untouched"""
    n, c_in, h, w = qx.shape
    c_out, _, kh, kw = qw.shape
    ho, wo = Q.out_hw(h, w, (kh, kw), stride, pad)
    px, pitch = n * ho * wo, Q.cpitch(c_in)
    dx, dw = ctx.upload(Q.nhwc(qx, pitch).view(np.uint8)), ctx.upload(Q.pack_weight(qw, pitch, 0x55).view(np.uint8))
    dps, dsx, dwp = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32)), ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wparams, f32))
    db = ctx.upload(qb.view(np.uint8)) if qb is not None else None
    dbp = ctx.upload(np.array(bparams, f32)) if qb is not None else None
    dsy = ctx.upload(np.array([sy], f32))
    qbuf = ctx.upload(np.full(px * pitch_y + 2 * GUARD, FILL, np.uint8))
    sbuf = ctx.upload(np.full(px + 2 * GUARD, FILL, np.int32))
    before = _in_use(ctx)
    ctx.call("th_conv2d_q8q8_fwd_codes", dx, pitch, dps, dsx, n, c_in, h, w, dw, c_out, kh, kw, stride[0], stride[1], pad[0], pad[1], dwp, db, dbp, relu,
             dsy, qbuf.offset(GUARD), pitch_y, sbuf.offset(4 * GUARD) if want_sums else None)
    assert _in_use(ctx) == before
    qraw, sraw = ctx.download(qbuf, (px * pitch_y + 2 * GUARD,), np.uint8), ctx.download(sbuf, (px + 2 * GUARD,), np.int32)
    assert (qraw[:GUARD] == FILL).all() and (qraw[GUARD + px * pitch_y:] == FILL).all(), "bytes around the codes were written"
    assert (sraw[:GUARD] == FILL).all() and (sraw[GUARD + px:] == FILL).all(), "words around the pixel sums were written"
    return qraw[GUARD:GUARD + px * pitch_y].view(np.int8).reshape(n, ho, wo, pitch_y), sraw[GUARD:GUARD + px].reshape(n, ho, wo)


def test_case_table_reaches_every_form_and_edge():
    assert_case_table_coverage()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_codes_padding_and_pixel_sums_are_the_reference_bit_for_bit(ctx, case):
    n, c_in, h, w, c_out, k, s, p = case
    qx, qw, qb = _operands(n, c_in, h, w, c_out, k, seed=2000 + CASES.index(case))
    # bias and ReLU each on and off; pixel sums asked for or not; the tightest pitch, then one with whole pieces beyond the channel tile
    for (sx, wp), (bias, relu, want_sums, extra) in zip(PARAMS + PARAMS, ((0, 0, 1, 0), (1, 0, 0, 0), (1, 1, 1, 32), (0, 1, 0, 16))):
        y = Q.conv_q8q8(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu)
        sy = f32(R.act_scale_of(y) * f32(0.6))          # the next layer's scale: the outer 40 % of the range saturates
        pitch_y = Q.cpitch(c_out) + extra
        ref_q, ref_ps = QC.conv_q8q8_codes(qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, sy, pitch_y)
        got_q, got_ps = _codes_call(ctx, qx, sx, qw, wp, qb if bias else None, BPARAMS, s, p, relu, sy, pitch_y, want_sums)
        what = str((case, sx, wp, "bias", bias, "relu", relu, "pitch", pitch_y))
        np.testing.assert_array_equal(got_q[..., :c_out], ref_q[..., :c_out], err_msg=what)
        assert not got_q[..., c_out:].any(), "padding bytes must be 0: " + what
        if want_sums:
            np.testing.assert_array_equal(got_ps, ref_ps, err_msg=what)
        else:
            assert (got_ps == FILL).all(), "pixel sums were written although none were asked for"
        if c_out * n * h * w >= 64:
            assert len(np.unique(ref_q[..., :c_out])) > 8 and np.abs(ref_q.astype(int)).max() >= 127      # the codes spread and saturate


def test_codes_do_not_depend_on_the_batch(ctx):
    n, c_in, h, w, c_out, k, s, p = 5, 15, 7, 11, 32, (3, 3), (1, 1), (1, 1)      # 77 pixels an image: every image starts at another place of a tile
    qx, qw, qb = _operands(n, c_in, h, w, c_out, k, seed=77)
    sx, wp = PARAMS[1]
    sy = f32(R.act_scale_of(Q.conv_q8q8(qx, sx, qw, wp, qb, BPARAMS, s, p, True)) * f32(0.6))
    whole_q, whole_ps = _codes_call(ctx, qx, sx, qw, wp, qb, BPARAMS, s, p, 1, sy, 32, True)
    for b in range(n):
        q1, ps1 = _codes_call(ctx, qx[b:b + 1], sx, qw, wp, qb, BPARAMS, s, p, 1, sy, 32, True)
        np.testing.assert_array_equal(q1[0], whole_q[b], err_msg=f"image {b} alone")
        np.testing.assert_array_equal(ps1[0], whole_ps[b], err_msg=f"image {b} alone")


def test_a_layer_wider_than_one_workgroup_is_refused_by_name(ctx):
    hip = _lib()
    n, c_in, h, w, k = 1, 16, 5, 5, (3, 3)
    qx, qw, _ = _operands(n, c_in, h, w, 129, k, seed=5)
    dx, dw = ctx.upload(Q.nhwc(qx, 16).view(np.uint8)), ctx.upload(Q.pack_weight(qw, 16).view(np.uint8))
    dps = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32))
    dsx, dwp, dsy = ctx.upload(np.array([1.0], f32)), ctx.upload(np.array([0.0, 1.0], f32)), ctx.upload(np.array([4000.0], f32))
    dq, dsum = ctx.upload(np.full(9 * 144 + 64, FILL, np.uint8)), ctx.upload(np.full(9, FILL, np.int32))
    good = dict(x=int(dx), cp=16, ps=int(dps), sx=int(dsx), co=128, sy=int(dsy), qy=int(dq), cpy=128, ys=int(dsum))

    def call(**kw):
        a = dict(good, **kw)
        return hip.th_conv2d_q8q8_fwd_codes(ctx.h, a["x"], a["cp"], a["ps"], a["sx"], n, c_in, h, w, int(dw), a["co"], 3, 3, 1, 1, 0, 0, int(dwp), None, None, 0,
                                            a["sy"], a["qy"], a["cpy"], a["ys"])

    before = _in_use(ctx)
    assert call(co=129, cpy=144) != 0
    assert b"th_conv2d_q8q8_fwd_codes" in hip.th_last_error() and b"129" in hip.th_last_error()
    for what, kw in (("null output scale", dict(sy=None)), ("null output codes", dict(qy=None)), ("null codes", dict(x=None)), ("null pixel sums", dict(ps=None)),
                     ("output codes off 16 bytes", dict(qy=int(dq) + 4)), ("cpitch_y % 16", dict(cpy=136)), ("cpitch_y below c_out", dict(cpy=112)),
                     ("x off 16 bytes", dict(x=int(dx) + 8)), ("cpitch below c_in", dict(cp=0)), ("c_out 0", dict(co=0))):
        assert call(**kw) != 0 and b"th_conv2d_q8q8_fwd_codes" in hip.th_last_error(), what
    assert _in_use(ctx) == before
    assert (ctx.download(dq, (9 * 144 + 64,), np.uint8) == FILL).all(), "a refused call wrote"
    assert call() == 0                                   # the next call succeeds: exactly the limit
    ref_q, ref_ps = QC.conv_q8q8_codes(qx, 1.0, qw[:128], (0.0, 1.0), None, None, (1, 1), (0, 0), False, 4000.0, 128)
    np.testing.assert_array_equal(ctx.download(dq, (1, 3, 3, 128), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(dsum, (1, 3, 3), np.int32), ref_ps)
    assert call(ys=None) == 0                            # pixel sums are optional


# ---------------------------------------------------------------- 2: the max-pool on codes
POOLS = [((2, 2), (2, 2), (0, 0)), ((3, 3), (2, 2), (1, 1)), ((3, 2), (2, 1), (2, 1))]


def _pool_call(ctx, q, c, k, s, p):
    n, h, w, pitch = q.shape
    ho, wo = Q.out_hw(h, w, k, s, p)
    px = n * ho * wo
    qbuf = ctx.upload(np.full(px * pitch + 2 * GUARD, FILL, np.uint8))
    sbuf = ctx.upload(np.full(px + 2 * GUARD, FILL, np.int32))
    dq = ctx.upload(q.view(np.uint8))
    before = _in_use(ctx)
    ctx.call("th_maxpool2d_nhwc_int8", dq, n, c, h, w, pitch, k[0], k[1], s[0], s[1], p[0], p[1], qbuf.offset(GUARD), sbuf.offset(4 * GUARD))
    assert _in_use(ctx) == before
    qraw, sraw = ctx.download(qbuf, (px * pitch + 2 * GUARD,), np.uint8), ctx.download(sbuf, (px + 2 * GUARD,), np.int32)
    assert (qraw[:GUARD] == FILL).all() and (qraw[GUARD + px * pitch:] == FILL).all(), "bytes around the codes were written"
    assert (sraw[:GUARD] == FILL).all() and (sraw[GUARD + px:] == FILL).all(), "words around the pixel sums were written"
    return qraw[GUARD:GUARD + px * pitch].view(np.int8).reshape(n, ho, wo, pitch), sraw[GUARD:GUARD + px].reshape(n, ho, wo)


# c: 1 -- 64 on both sides of a 16-byte piece; 1040 = 65 pieces, one more than a wave of lanes takes in one turn (a 3 x 3 map there)
@pytest.mark.parametrize("c", [1, 15, 16, 17, 64, 1040])
def test_max_pool_on_codes_is_the_reference(ctx, c):
    rng = np.random.default_rng(300 + c)
    for h, w in ((7, 7), (9, 11)) if c <= 64 else ((3, 3),):
        for n in (1, 3):
            for extra in (0, 16):      # the tightest pitch, and one whose piece count is no power of two for c <= 32
                q = rng.integers(-128, 128, (n, h, w, Q.cpitch(c) + extra)).astype(np.int8)      # the padding bytes hold anything
                q[0, 0, 0, 0], q[-1, -1, -1, c - 1] = -128, 127
                for k, s, p in POOLS:
                    ref_q, ref_ps = QC.max_pool_codes(q, c, k, s, p)
                    got_q, got_ps = _pool_call(ctx, q, c, k, s, p)
                    what = str((c, n, h, w, extra, k, s, p))
                    np.testing.assert_array_equal(got_q, ref_q, err_msg=what)
                    np.testing.assert_array_equal(got_ps, ref_ps, err_msg=what)


def test_max_pool_refusals_name_the_function_and_the_next_call_succeeds(ctx):
    hip = _lib()
    q = np.random.default_rng(4).integers(-128, 128, (2, 6, 5, 32)).astype(np.int8)
    dq, dy, ds = ctx.upload(q.view(np.uint8)), ctx.upload(np.full(2 * 3 * 2 * 32 + 64, FILL, np.uint8)), ctx.upload(np.full(12, FILL, np.int32))
    good = dict(q=int(dq), n=2, c=17, h=6, w=5, cp=32, kh=2, kw=2, sh=2, sw=2, ph=0, pw=0, y=int(dy), s=int(ds))

    def call(**kw):
        a = dict(good, **kw)
        return hip.th_maxpool2d_nhwc_int8(ctx.h, *[a[f] for f in ("q", "n", "c", "h", "w", "cp", "kh", "kw", "sh", "sw", "ph", "pw", "y", "s")])

    before = _in_use(ctx)
    for what, kw in (("null codes", dict(q=None)), ("null output", dict(y=None)), ("null pixel sums", dict(s=None)), ("codes off 16 bytes", dict(q=int(dq) + 4)),
                     ("output off 16 bytes", dict(y=int(dy) + 8)), ("cpitch % 16", dict(cp=24)), ("cpitch below c", dict(c=33)), ("n < 0", dict(n=-1)),
                     ("c 0", dict(c=0)), ("h 0", dict(h=0)), ("w 0", dict(w=0)), ("k_h 0", dict(kh=0)), ("k_w 0", dict(kw=0)), ("stride 0", dict(sw=0)),
                     ("negative padding", dict(ph=-1)), ("an empty output map", dict(kh=7)), ("an empty output map", dict(kw=6))):
        assert call(**kw) != 0 and b"th_maxpool2d_nhwc_int8" in hip.th_last_error(), what
    assert hip.th_maxpool2d_nhwc_int8(None, *[good[f] for f in ("q", "n", "c", "h", "w", "cp", "kh", "kw", "sh", "sw", "ph", "pw", "y", "s")]) != 0
    assert _in_use(ctx) == before
    assert (ctx.download(dy, (2 * 3 * 2 * 32 + 64,), np.uint8) == FILL).all(), "a refused call wrote"
    assert call(n=0) == 0                                # an empty batch is a shape: nothing is launched
    assert call() == 0
    ref_q, ref_ps = QC.max_pool_codes(q, 17, (2, 2), (2, 2))
    np.testing.assert_array_equal(ctx.download(dy, (2, 3, 2, 32), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(ds, (2, 3, 2), np.int32), ref_ps)


# ---------------------------------------------------------------- 3: the chained twin is the unchained twin, bit for bit
def _small_cnn(rng):      # tests/test_gpu_qconv.py's CNN
    import taper_amd as T
    model = T.Sequential([T.Conv2dReLU(1, 4, (3, 3)), T.MaxPool2d((2, 2), (2, 2)), T.Conv2d(4, 8, (3, 3), None, (1, 1)), T.ReLU(), T.MaxPool2d((2, 2), (2, 2)),
                          T.Flatten(1), T.Linear(8 * 2 * 2, 10, True)])
    for p in model.parameters():
        p.set_data((0.4 * rng.standard_normal(p.numel())).astype(f32))
    return model


# name -> (model, input shape, links)
MODELS = {
    "cnn_reference-b3": (lambda rng: B.get("hip").sequential(B.nonzero_biases(B.cnn_reference(rng), rng)), (3, 1, 28, 28), 4),
    "cnn_simple-b2": (lambda rng: B.get("hip").sequential(B.nonzero_biases(B.cnn_simple(rng), rng)), (2, 1, 28, 28), 1),
    "cnn_simple-b3": (lambda rng: B.get("hip").sequential(B.nonzero_biases(B.cnn_simple(rng), rng)), (3, 1, 28, 28), 1),
    "small_cnn-b8": (_small_cnn, (8, 1, 12, 12), 1),
}


def _twins(model, calib):
    return model.quantize_static_chain(calib), model.quantize_static_conv(calib)


def _assert_same_twin(chain, plain):
    np.testing.assert_array_equal(_bits(chain.act_scales()), _bits(plain.act_scales()))
    assert chain.storage_bytes() == plain.storage_bytes() and plain.chain_links() == 0
    ta, tb = chain.tensors(), plain.tensors()
    assert len(ta) == len(tb)
    for (k1, c1, p1), (k2, c2, p2) in zip(ta, tb):
        assert k1 == k2
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))


@pytest.mark.parametrize("name", list(MODELS))
def test_chained_twin_is_the_unchained_twin_bit_for_bit(name):
    import taper_amd as T
    build, shape, links = MODELS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    model = build(rng)
    calib = [T.Tensor(a, shape) for a in (rng.uniform(0, 1, shape).astype(f32), (1.5 * rng.standard_normal(shape)).astype(f32))]
    T.Tape.reset()
    chain, plain = _twins(model, calib)
    assert T.Tape.len() == 0
    assert chain.chain_links() == links
    _assert_same_twin(chain, plain)
    x = rng.standard_normal(shape).astype(f32)
    far = (3 * 1.5 * 4 * np.sign(x)).astype(f32)          # beyond the calibration range: the first codes saturate
    far[:, :, :, ::3] = x[:, :, :, ::3]
    before = _pool_in_use()
    refs = {}
    for key, data in (("x", x), ("far", far)):
        y = chain(T.Tensor(data, shape).requires_grad())
        assert T.Tape.len() == 0 and y.tape_node() == 0
        got = y.data()
        del y
        assert _pool_in_use() == before                  # codes, pixel sums and every map went back to the pool
        refs[key] = plain(T.Tensor(data, shape)).data()
        assert np.isfinite(refs[key]).all() and np.abs(refs[key]).max() > 0
        np.testing.assert_array_equal(_bits(got), _bits(refs[key]), err_msg=key)
    for b in (0, shape[0] - 1):                           # an image's result does not depend on its batch
        alone = chain(T.Tensor(x[b:b + 1], (1,) + shape[1:])).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(refs["x"][b]), err_msg=f"image {b} alone")
    assert _pool_in_use() == before


# ---------------------------------------------------------------- 4: links that break
def _randomize(model, rng, scale=0.3):
    for p in model.parameters():
        p.set_data((scale * rng.standard_normal(p.numel())).astype(f32))
    return model


def _c3(T, ci, co, relu=True):
    return (T.Conv2dReLU if relu else T.Conv2d)(ci, co, (3, 3), None, (1, 1))


def _pool(T):
    return T.MaxPool2d((2, 2), (2, 2))


# (what, layers, input shape, links)
VARIANTS = [
    ("a 160-channel conv ahead of a conv", lambda T: [_c3(T, 2, 160), _c3(T, 160, 8), _c3(T, 8, 4)], (2, 2, 6, 6), 1),
    ("conv, pool, ReLU, conv", lambda T: [_c3(T, 2, 8, False), _pool(T), T.ReLU(), _c3(T, 8, 4)], (2, 2, 8, 8), 0),
    ("conv, ReLU, pool, conv", lambda T: [_c3(T, 2, 8, False), T.ReLU(), _pool(T), _c3(T, 8, 4)], (2, 2, 8, 8), 1),
    ("two pools between two convs", lambda T: [_c3(T, 2, 8), _pool(T), _pool(T), _c3(T, 8, 4)], (2, 2, 8, 8), 0),
    ("a sigmoid between two convs", lambda T: [_c3(T, 2, 8, False), T.Sigmoid(), _c3(T, 8, 4)], (2, 2, 6, 6), 0),
    ("a grouped conv in the middle", lambda T: [_c3(T, 2, 4), T.Conv2d(4, 8, (3, 3), None, (1, 1), None, 2), T.ReLU(), _c3(T, 8, 4)], (2, 2, 6, 6), 0),
    ("a 5 x 5 conv in the middle, then a link", lambda T: [_c3(T, 2, 4), T.Conv2dReLU(4, 8, (5, 5), None, (2, 2)), _c3(T, 8, 8), _pool(T), _c3(T, 8, 4)],
     (2, 2, 8, 8), 1),
    ("a padded 3 x 3 / 2 pool, 17 channels", lambda T: [_c3(T, 3, 17), T.MaxPool2d((3, 3), (2, 2), (1, 1)), _c3(T, 17, 5, False)], (3, 3, 9, 7), 1),
    ("a pool with the default stride", lambda T: [_c3(T, 1, 6), T.MaxPool2d((2, 2)), _c3(T, 6, 6), T.Flatten(1), T.Linear(6 * 16, 10, True)], (2, 1, 8, 8), 1),
    ("a nested Sequential", lambda T: [T.Sequential([_c3(T, 2, 8), _c3(T, 8, 8)]), _pool(T), T.Sequential([_c3(T, 8, 4), _c3(T, 4, 4)])], (2, 2, 8, 8), 2),
]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0].replace(" ", "_") for v in VARIANTS])
def test_links_that_break_and_links_that_hold(variant):
    import taper_amd as T
    name, layers, shape, links = variant
    rng = np.random.default_rng(sum(map(ord, name)))
    model = _randomize(T.Sequential(layers(T)), rng)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    chain, plain = _twins(model, calib)
    assert chain.chain_links() == links
    _assert_same_twin(chain, plain)
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    before = _pool_in_use()
    got, ref = chain(x).data(), plain(x).data()
    assert _pool_in_use() == before
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(_bits(got), _bits(ref))


def test_on_a_linear_only_model_it_is_quantize_static():
    import taper_amd as T
    rng = np.random.default_rng(62)
    model = T.Sequential([T.Linear(100, 40, True, seed=5), T.ReLU(), T.Linear(40, 10, True, seed=6)])
    calib = [T.Tensor(rng.standard_normal((16, 100)).astype(f32), (16, 100)) for _ in range(2)]
    a, b = model.quantize_static_chain(calib), model.quantize_static(calib)
    assert a.chain_links() == 0 and b.chain_links() == 0 and model.quantize("int8").chain_links() == 0
    _assert_same_twin(a, b)
    x = T.Tensor(rng.standard_normal((37, 100)).astype(f32), (37, 100))
    np.testing.assert_array_equal(_bits(a(x).data()), _bits(b(x).data()))


def test_qat_convs_deploy_as_their_inner_layers():
    import taper_amd as T
    rng = np.random.default_rng(63)
    shape = (4, 3, 8, 8)
    calib = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    plain = T.Sequential([T.Conv2dReLU(3, 8, (3, 3), None, (1, 1), seed=3), T.MaxPool2d((2, 2), (2, 2)), T.Conv2dReLU(8, 8, (3, 3), None, (1, 1), seed=5),
                          T.Flatten(1), T.Linear(8 * 16, 10, True, seed=4)])
    qat_model = T.Sequential([T.QATConv2d(3, 8, (3, 3), None, (1, 1), relu=True, seed=3), T.MaxPool2d((2, 2), (2, 2)),
                              T.QATConv2d(8, 8, (3, 3), None, (1, 1), relu=True, seed=5), T.Flatten(1), T.QATLinear(8 * 16, 10, True, seed=4)])
    for a, b in zip(plain.parameters(), qat_model.parameters()):
        np.testing.assert_array_equal(_bits(a.data()), _bits(b.data()))
    ref = plain.quantize_static_conv(calib)
    T.qat.enable()
    try:
        T.Tape.reset()
        q = qat_model.quantize_static_chain(calib)
        assert T.Tape.len() == 0
    finally:
        T.qat.disable()
    assert q.chain_links() == 1 and q.act_scales().shape == (3,)
    _assert_same_twin(q, ref)
    x = T.Tensor(rng.standard_normal(shape).astype(f32), shape)
    np.testing.assert_array_equal(_bits(q(x).data()), _bits(ref(x).data()))


def test_chain_refusals_are_static_convs_and_leak_nothing():
    import taper_amd as T
    shape = (2, 1, 12, 12)
    x = T.Tensor(np.zeros(shape, f32), shape)
    model = _small_cnn(np.random.default_rng(64))
    dropout = T.Sequential([T.Conv2d(1, 4, (3, 3)), T.Dropout(0.5)])
    wide = T.Sequential([T.Conv2d(7282, 1, (3, 3), bias=False)])      # 7282 * 9 = 65538
    T.Device.sync()
    before = _pool_in_use()
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static_chain(x)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        model.quantize_static_chain([])
    with pytest.raises(T.TaperError, match="undefined calibration tensor"):
        model.quantize_static_chain([x, None])
    with pytest.raises(T.TaperError, match="65538"):
        wide.quantize_static_chain(T.Tensor(np.zeros((1, 7282, 3, 3), f32), (1, 7282, 3, 3)))
    assert _pool_in_use() == before
    q = model.quantize_static_chain(x)                   # and the next valid call succeeds
    assert q.act_scales().shape == (3,) and q.chain_links() == 1
    held = _pool_in_use()
    with pytest.raises(T.TaperError, match="in_channels"):      # a forward refused halfway gives its buffers back
        q(T.Tensor(np.zeros((2, 3, 12, 12), f32), (2, 3, 12, 12)))
    assert _pool_in_use() == held
    assert q(x).data().shape == (2, 10)
