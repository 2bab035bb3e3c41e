"""A skip connection in the int8 conv epilogue on the GPU: th_conv2d_q8q8_fwd_residual and th_conv2d_q8q8_fwd_codes_residual in
all 24 kernel forms (NT 1 / 2 / 4 x f32 / codes destination x one weight pair / one per channel x an f32 / a codes residual) against the
numpy restatement of tests/qres_ref.py.  The integer sums are exact and every f32 operation rounds once, so every comparison is on bits."""
import numpy as np
import pytest

from tests import qconv_ref as Q
from tests import qres_ref as S
from tests import qstatic_ref as R
from tests import test_gpu_qbn as TB
from tests import test_gpu_qconv as TC
from tests import test_gpu_qperchan as TP

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, GUARD_BITS = TC.GUARD, TC.GUARD_BITS      # words on either side of an f32 map
BG, FILL = 256, 0x55                             # bytes on either side of a code map (words: of the pixel sums); what padding and outputs hold before
BPARAMS = TC.BPARAMS
_bits, _in_use, _lib = TC._bits, TC._in_use, TC._lib
F32_FN, CODES_FN = "th_conv2d_q8q8_fwd_residual", "th_conv2d_q8q8_fwd_codes_residual"


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


# (n, c_in, h, w, c_out).  With 3x3 / stride 1 / pad 1: 128 pixels = exactly a pixel tile across both images, c_out off 4 in the
# 32-channel form; 30 pixels, the 64-channel form one past a tile; 105 pixels across three images, one past two tiles in the 128-channel
# form; 49 pixels by exactly 128 channels; two channel tiles (f32 destination only); 162 pixels = two pixel tiles, c_out off 16 and 32.
SHAPES = [(2, 3, 8, 8, 31), (1, 16, 6, 5, 33), (3, 8, 5, 7, 65), (1, 64, 7, 7, 128), (2, 16, 6, 5, 130), (2, 4, 9, 9, 20)]
GEOMS = [((3, 3), (1, 1), (1, 1)), ((1, 1), (1, 1), (0, 0)), ((3, 3), (2, 2), (1, 1))]      # (k, stride, pad): the convs a block's twin runs
CASES = [(s, g) for s in SHAPES for g in GEOMS]
IDS = ["n{}-c{}-{}x{}-o{}-k{}s{}".format(*s, g[0][0], g[1][0]) for s, g in CASES]


def test_case_table_reaches_every_form_and_edge():
    forms = set()
    for (n, c_in, h, w, c_out), (k, s, p) in CASES:
        pl = TC.plan(n, c_in, h, w, c_out, k, s, p)
        for codes in ((0, 1) if c_out <= 128 else (0,)):
            for pc in (0, 1):
                for res in (1, 2):
                    forms.add((pl["nt"], codes, pc, res))
    assert len(forms) == 24
    pl = {s[4]: TC.plan(*s[:4], s[4], *GEOMS[0]) for s in SHAPES}
    assert [pl[c]["nt"] for c in (31, 33, 65, 128, 130, 20)] == [1, 2, 4, 4, 4, 1]
    assert pl[130]["tiles_n"] == 2 and pl[20]["tiles_m"] == 2 and pl[31]["tiles_m"] == 1 and 2 * 8 * 8 == pl[31]["tile_m"]
    assert TC.plan(3, 8, 5, 7, 65, *GEOMS[2])["h_out"] == 3      # stride 2: the residual has the output's shape, not the input's


class _Operands:
    """the uploaded operands of one shape and geometry, shared by every call on it"""

    def __init__(self, ctx, shape, geom, seed):
        n, c_in, h, w, c_out = shape
        self.k, self.s, self.p = geom
        self.shape, self.c_out = shape, c_out
        self.qx, self.qw, self.qb = TC._operands(n, c_in, h, w, c_out, self.k, seed)
        self.pitch = Q.cpitch(c_in)
        self.ho, self.wo = Q.out_hw(h, w, self.k, self.s, self.p)
        self.oshape = (n, c_out, self.ho, self.wo)
        self.dx, self.dw = ctx.upload(Q.nhwc(self.qx, self.pitch).view(np.uint8)), ctx.upload(Q.pack_weight(self.qw, self.pitch, FILL).view(np.uint8))
        self.dps = ctx.upload(self.qx.astype(np.int64).sum(axis=1).astype(np.int32))
        self.db, self.dbp = ctx.upload(self.qb.view(np.uint8)), ctx.upload(np.array(BPARAMS, f32))

    def head(self, dsx, dwp, bias, relu):
        n, c_in, h, w, c_out = self.shape
        return (self.dx, self.pitch, self.dps, dsx, n, c_in, h, w, self.dw, c_out, self.k[0], self.k[1], self.s[0], self.s[1], self.p[0], self.p[1], dwp,
                self.db if bias else None, self.dbp if bias else None, relu)


def _residual_args(ctx, res, res_q, res_scale, cpitch_r):
    """-> (the four residual arguments, a check that the guards around the residual came back intact)"""
    if res is not None:
        buf = ctx.upload(np.concatenate([np.full(GUARD, GUARD_BITS, np.uint32), _bits(res).reshape(-1), np.full(GUARD, GUARD_BITS, np.uint32)]))

        def intact():
            raw = ctx.download(buf, (res.size + 2 * GUARD,), np.uint32)
            assert (raw[:GUARD] == GUARD_BITS).all() and (raw[GUARD + res.size:] == GUARD_BITS).all() and np.array_equal(raw[GUARD:GUARD + res.size], _bits(res).reshape(-1))
        return (buf.offset(4 * GUARD), None, 0, None), intact, buf
    rows = Q.nhwc(res_q, cpitch_r, FILL).view(np.uint8).reshape(-1)      # every padding byte of a row is 0x55
    host = np.concatenate([np.full(BG, FILL, np.uint8), rows, np.full(BG, FILL, np.uint8)])
    buf, dsr = ctx.upload(host), ctx.upload(np.array([res_scale], f32))

    def intact():
        assert np.array_equal(ctx.download(buf, host.shape, np.uint8), host)
    return (None, buf.offset(BG), cpitch_r, dsr), intact, (buf, dsr)


def _f32_call(ctx, ops, sx, wp, bias, relu, ab, pc, res=None, res_q=None, res_scale=None, cpitch_r=0, graph=False):
    total = int(np.prod(ops.oshape))
    dsx, dwp, dab = ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wp, f32)), ctx.upload(np.asarray(ab, f32))
    rargs, intact, keep = _residual_args(ctx, res, res_q, res_scale, cpitch_r)
    ybuf = ctx.upload(np.full(total + 2 * GUARD, GUARD_BITS, np.uint32))
    y = ybuf.offset(4 * GUARD)
    ctx.call("th_fill_f32", y, float("nan"), total)
    before = _in_use(ctx)
    args = ops.head(dsx, dwp, bias, relu) + (y, pc, dab) + rargs
    if graph:
        ctx.graph_begin()
        ctx.call(F32_FN, *args)
        g = ctx.graph_end()
        ctx.graph_launch(g)
        ctx.sync()
        ctx.graph_destroy(g)
    else:
        ctx.call(F32_FN, *args)
        assert _in_use(ctx) == before
    out = ctx.download(ybuf, (total + 2 * GUARD,), np.uint32)
    assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + total:] == GUARD_BITS).all(), "words around the output were written"
    intact()
    return out[GUARD:GUARD + total].view(f32).reshape(ops.oshape)


def _codes_call(ctx, ops, sx, wp, bias, relu, ab, pc, sy, pitch_y, want_sums, res=None, res_q=None, res_scale=None, cpitch_r=0, graph=False):
    n, c_out, ho, wo = ops.oshape
    px = n * ho * wo
    dsx, dwp, dab, dsy = ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wp, f32)), ctx.upload(np.asarray(ab, f32)), ctx.upload(np.array([sy], f32))
    rargs, intact, keep = _residual_args(ctx, res, res_q, res_scale, cpitch_r)
    qbuf = ctx.upload(np.full(px * pitch_y + 2 * BG, FILL, np.uint8))
    sbuf = ctx.upload(np.full(px + 2 * BG, FILL, np.int32))
    before = _in_use(ctx)
    args = ops.head(dsx, dwp, bias, relu) + (dsy, qbuf.offset(BG), pitch_y, sbuf.offset(4 * BG) if want_sums else None, pc, dab) + rargs
    if graph:
        ctx.graph_begin()
        ctx.call(CODES_FN, *args)
        g = ctx.graph_end()
        ctx.graph_launch(g)
        ctx.sync()
        ctx.graph_destroy(g)
    else:
        ctx.call(CODES_FN, *args)
        assert _in_use(ctx) == before
    qraw, sraw = ctx.download(qbuf, (px * pitch_y + 2 * BG,), np.uint8), ctx.download(sbuf, (px + 2 * BG,), np.int32)
    assert (qraw[:BG] == FILL).all() and (qraw[BG + px * pitch_y:] == FILL).all(), "bytes around the codes were written"
    assert (sraw[:BG] == FILL).all() and (sraw[BG + px:] == FILL).all(), "words around the pixel sums were written"
    intact()
    return qraw[BG:BG + px * pitch_y].view(np.int8).reshape(n, ho, wo, pitch_y), sraw[BG:BG + px].reshape(n, ho, wo)


def _pair_sets(c_out, pc):
    """(sx, weight pairs, affine, residual scale): pure integers (they pin the lane maps and the byte of every code), then floats"""
    if pc:
        return [(1.0, TP.int_pairs(c_out), TB.int_affine(c_out), 1.0), (0.0173, TP.float_pairs(c_out), TB.float_affine(c_out), 0.0371)]
    return [(TC.PARAMS[0][0], TC.PARAMS[0][1], TB.int_affine(c_out), 1.0), (TC.PARAMS[1][0], TC.PARAMS[1][1], TB.float_affine(c_out), 0.0371)]


def _residuals(rng, oshape, k):
    """a codes residual over the full range with -128 and 127 in it, and an f32 one: integer-valued for the integer set, else of the values' size"""
    res_q = rng.integers(-128, 128, oshape).astype(np.int8)
    res_q.reshape(-1)[0], res_q.reshape(-1)[-1] = 127, -128
    res = (rng.integers(-1000, 1001, oshape).astype(f32) if k == 0 else (3 * rng.standard_normal(oshape)).astype(f32))
    return res, res_q


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_residual_products_are_the_reference_bit_for_bit(ctx, case):
    shape, geom = case
    i = CASES.index(case)
    ops = _Operands(ctx, shape, geom, seed=3000 + i)
    c_out = ops.c_out
    rng = np.random.default_rng(4000 + i)
    calls = 0
    for pc in (0, 1):
        sets = _pair_sets(c_out, pc)
        for k, bias, relu in ((0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)):
            sx, wp, ab, sr = sets[k]
            res, res_q = _residuals(rng, ops.oshape, k)
            plain = TB.N.conv_q8q8_affine(ops.qx, sx, ops.qw, wp, ops.qb if bias else None, BPARAMS, ops.s, ops.p, relu, ab, pc)
            for mode in (1, 2):
                calls += 1
                cpitch_r = Q.cpitch(c_out) + (0, 16, 48)[calls % 3]      # the tightest pitch and two looser ones
                kw = dict(res=res) if mode == 1 else dict(res_q=res_q, res_scale=sr)
                gkw = dict(kw, cpitch_r=cpitch_r) if mode == 2 else kw
                what = str((case, "pc", pc, "set", k, "bias", bias, "relu", relu, "res", mode, "cpitch_r", cpitch_r))
                ref = S.conv_q8q8_residual(ops.qx, sx, ops.qw, wp, ops.qb if bias else None, BPARAMS, ops.s, ops.p, relu, ab, pc, **kw)
                assert not np.isnan(ref).any() and not np.array_equal(ref, plain), what      # the residual reaches the value
                got = _f32_call(ctx, ops, sx, wp, bias, relu, ab, pc, **gkw)
                np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=what)
                if c_out > 128:
                    continue
                sy = f32(R.act_scale_of(ref) * f32(0.6))      # the next layer's scale: the outer 40 % of the range saturates
                pitch_y = Q.cpitch(c_out) + (0, 16)[calls % 2]
                want_sums = (calls // 2) % 2
                ref_q, ref_ps = S.conv_q8q8_codes_residual(ops.qx, sx, ops.qw, wp, ops.qb if bias else None, BPARAMS, ops.s, ops.p, relu, ab, pc, sy, pitch_y, **kw)
                got_q, got_ps = _codes_call(ctx, ops, sx, wp, bias, relu, ab, pc, sy, pitch_y, want_sums, **gkw)
                np.testing.assert_array_equal(got_q[..., :c_out], ref_q[..., :c_out], err_msg=what)
                assert not got_q[..., c_out:].any(), "padding bytes must be 0: " + what
                if want_sums:
                    np.testing.assert_array_equal(got_ps, ref_ps, err_msg=what)
                else:
                    assert (got_ps == FILL).all(), "pixel sums were written although none were asked for"
    assert calls == 16


def test_a_zero_residual_gives_the_affine_entrys_values(ctx):
    ops = _Operands(ctx, (3, 8, 5, 7, 65), GEOMS[0], seed=77)
    sx, wp, ab, _ = _pair_sets(65, 1)[1]
    for relu in (0, 1):
        ref = TB.N.conv_q8q8_affine(ops.qx, sx, ops.qw, wp, ops.qb, BPARAMS, ops.s, ops.p, relu, ab, 1)
        a = _f32_call(ctx, ops, sx, wp, 1, relu, ab, 1, res=np.zeros(ops.oshape, f32))
        b = _f32_call(ctx, ops, sx, wp, 1, relu, ab, 1, res_q=np.zeros(ops.oshape, np.int8), res_scale=0.5, cpitch_r=80)
        assert np.array_equal(a, ref) and np.array_equal(b, ref)      # as values: -0 + 0 is +0


def test_nan_and_infinities_in_the_residual_follow_the_relu_and_codec_rules(ctx):
    """max(NaN, 0) = 0 and the code of NaN is 0; +inf stays (code 127), -inf goes to 0 under the ReLU (code -128 without it).  A codes
    residual with an infinite scale gives +-inf, and NaN where the code is 0."""
    ops = _Operands(ctx, (1, 16, 6, 5, 33), GEOMS[0], seed=78)
    sx, wp, ab, _ = _pair_sets(33, 0)[1]
    rng = np.random.default_rng(79)
    res = rng.standard_normal(ops.oshape).astype(f32)
    flat = res.reshape(-1)
    flat[::7], flat[1::11], flat[2::13] = np.nan, np.inf, -np.inf
    res_q = rng.integers(-128, 128, ops.oshape).astype(np.int8)
    res_q.reshape(-1)[::5] = 0
    for relu in (0, 1):
        for kw in (dict(res=res), dict(res_q=res_q, res_scale=float("inf"))):
            gkw = dict(kw, cpitch_r=48) if "res_q" in kw else kw
            ref = S.conv_q8q8_residual(ops.qx, sx, ops.qw, wp, ops.qb, BPARAMS, ops.s, ops.p, relu, ab, 0, **kw)
            assert np.isnan(ref).any() != bool(relu) and np.isposinf(ref).any() and np.isneginf(ref).any() != bool(relu)
            got = _f32_call(ctx, ops, sx, wp, 1, relu, ab, 0, **gkw)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
            np.testing.assert_array_equal(_bits(got)[~np.isnan(ref)], _bits(ref)[~np.isnan(ref)])
            sy = f32(0.05)
            ref_q, ref_ps = S.conv_q8q8_codes_residual(ops.qx, sx, ops.qw, wp, ops.qb, BPARAMS, ops.s, ops.p, relu, ab, 0, sy, 48, **kw)
            got_q, got_ps = _codes_call(ctx, ops, sx, wp, 1, relu, ab, 0, sy, 48, 1, **gkw)
            np.testing.assert_array_equal(got_q, ref_q)
            np.testing.assert_array_equal(got_ps, ref_ps)
            nan = np.isnan(ref).transpose(0, 2, 3, 1)
            assert (ref_q[..., :33][nan] == 0).all() and (ref_q[..., :33][np.isposinf(ref).transpose(0, 2, 3, 1)] == 127).all()


def test_a_captured_graph_replays_the_eager_bits(ctx):
    ops = _Operands(ctx, (3, 8, 5, 7, 65), GEOMS[2], seed=80)
    sx, wp, ab, sr = _pair_sets(65, 1)[1]
    res, res_q = _residuals(np.random.default_rng(81), ops.oshape, 1)
    eager = _f32_call(ctx, ops, sx, wp, 1, 1, ab, 1, res_q=res_q, res_scale=sr, cpitch_r=80)
    replay = _f32_call(ctx, ops, sx, wp, 1, 1, ab, 1, res_q=res_q, res_scale=sr, cpitch_r=80, graph=True)
    np.testing.assert_array_equal(_bits(replay), _bits(eager))
    sy = f32(R.act_scale_of(eager) * f32(0.6))
    eq, es = _codes_call(ctx, ops, sx, wp, 1, 1, ab, 1, sy, 80, 1, res=res)
    gq, gs = _codes_call(ctx, ops, sx, wp, 1, 1, ab, 1, sy, 80, 1, res=res, graph=True)
    np.testing.assert_array_equal(gq, eq)
    np.testing.assert_array_equal(gs, es)
    assert len(np.unique(eq)) > 8


def test_refusals_name_the_function_launch_nothing_and_the_next_call_succeeds(ctx):
    hip = _lib()
    n, c_in, h, w = 1, 16, 5, 5
    qx, qw, _ = TC._operands(n, c_in, h, w, 129, (3, 3), seed=5)
    dqx, dqw = ctx.upload(Q.nhwc(qx, 16).view(np.uint8)), ctx.upload(Q.pack_weight(qw, 16).view(np.uint8))
    dps = ctx.upload(qx.astype(np.int64).sum(axis=1).astype(np.int32))
    dsx, dwp, dsy, dab = ctx.upload(np.array([1.0], f32)), ctx.upload(TP.int_pairs(129)), ctx.upload(np.array([90000.0], f32)), ctx.upload(TB.int_affine(129))
    dq, dsum = ctx.upload(np.full(9 * 144 + 64, FILL, np.uint8)), ctx.upload(np.full(9, FILL, np.int32))
    dyf = ctx.upload(np.full(9 * 129, GUARD_BITS, np.uint32))
    rng = np.random.default_rng(6)
    res = rng.integers(-50, 51, (1, 129, 3, 3)).astype(f32)
    res_q = rng.integers(-128, 128, (1, 129, 3, 3)).astype(np.int8)
    dres, dres_q, dsr = ctx.upload(res), ctx.upload(Q.nhwc(res_q, 144, FILL).view(np.uint8)), ctx.upload(np.array([2.0], f32))
    F, Qr, Sr = int(dres), int(dres_q), int(dsr)

    def codes(co=128, cpy=128, ab=int(dab), r=(F, None, 0, None)):
        return hip.th_conv2d_q8q8_fwd_codes_residual(ctx.h, int(dqx), 16, int(dps), int(dsx), n, c_in, h, w, int(dqw), co, 3, 3, 1, 1, 0, 0, int(dwp), None, None, 0,
                                                     int(dsy), int(dq), cpy, int(dsum), 1, ab, *r)

    def plain(co=129, ab=int(dab), cpitch=16, y=int(dyf), k=3, r=(None, Qr, 144, Sr)):
        return hip.th_conv2d_q8q8_fwd_residual(ctx.h, int(dqx), cpitch, int(dps), int(dsx), n, c_in, h, w, int(dqw), co, k, k, 1, 1, 0, 0, int(dwp), None, None, 0, y,
                                               1, ab, *r)

    before = _in_use(ctx)
    for fn, name in ((codes, CODES_FN), (plain, F32_FN)):
        name = name.encode()
        assert fn(ab=None) != 0 and name in hip.th_last_error() and b"null" in hip.th_last_error()
        assert fn(r=(F, Qr, 144, Sr)) != 0 and name in hip.th_last_error() and b"exactly one of d_res" in hip.th_last_error()
        assert fn(r=(None, None, 0, None)) != 0 and name in hip.th_last_error() and b"exactly one of d_res" in hip.th_last_error()
        assert fn(r=(None, Qr, 144, None)) != 0 and name in hip.th_last_error() and b"d_res_scale" in hip.th_last_error()
        assert fn(r=(None, Qr, 136, Sr)) != 0 and name in hip.th_last_error() and b"cpitch_r 136" in hip.th_last_error()      # no multiple of 16
        assert fn(r=(None, Qr, 112, Sr)) != 0 and name in hip.th_last_error() and b"cpitch_r 112" in hip.th_last_error()      # below c_out
        assert fn(r=(None, Qr + 8, 144, Sr)) != 0 and name in hip.th_last_error() and b"16-byte aligned" in hip.th_last_error()
    # the affine twins' refusals under the new names
    assert codes(129, 144) != 0 and CODES_FN.encode() in hip.th_last_error() and b"129" in hip.th_last_error()
    assert codes(128, 120) != 0 and CODES_FN.encode() in hip.th_last_error()
    for kw in (dict(cpitch=24), dict(y=None), dict(co=0), dict(k=6)):
        assert plain(**kw) != 0 and F32_FN.encode() in hip.th_last_error(), kw
    assert hip.th_conv2d_q8q8_fwd_residual(None, int(dqx), 16, int(dps), int(dsx), n, c_in, h, w, int(dqw), 129, 3, 3, 1, 1, 0, 0, int(dwp), None, None, 0, int(dyf), 1,
                                           int(dab), F, None, 0, None) != 0
    assert _in_use(ctx) == before
    assert (ctx.download(dq, (9 * 144 + 64,), np.uint8) == FILL).all() and (ctx.download(dyf, (9 * 129,), np.uint32) == GUARD_BITS).all(), "a refused call wrote"
    assert codes() == 0 and plain() == 0      # the next calls succeed
    ref_q, ref_ps = S.conv_q8q8_codes_residual(qx, 1.0, qw[:128], TP.int_pairs(128), None, None, (1, 1), (0, 0), False, TB.int_affine(128), 1, 90000.0, 128,
                                               res=res[:, :128])
    np.testing.assert_array_equal(ctx.download(dq, (1, 3, 3, 128), np.int8), ref_q)
    np.testing.assert_array_equal(ctx.download(dsum, (1, 3, 3), np.int32), ref_ps)
    ref = S.conv_q8q8_residual(qx, 1.0, qw, TP.int_pairs(129), None, None, (1, 1), (0, 0), False, TB.int_affine(129), 1, res_q=res_q, res_scale=2.0)
    np.testing.assert_array_equal(_bits(ctx.download(dyf, (1, 129, 3, 3))), _bits(ref))
