"""Calibrated int8 inference on the GPU (csrc/qgemm_i8.hip, Module.quantize_static): the integer-matrix-core product, the activation
codec and the static twin against the numpy restatement of tests/qstatic_ref.py.  The accumulator is an exact int32 and the epilogue is
four f32 operations rounded once each, so every comparison with the reference is on bits."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests import qstatic_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
RTOL = 1e-4
GUARD = 64                 # words on either side of an output
GUARD_BITS = 0xFFA5C3E1    # a NaN payload no computation produces


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


def _up16(k):
    return -(-k // 16) * 16


def _padded(codes, pitch, fill=0):
    rows, k = codes.shape
    out = np.full((rows, pitch), fill, np.int8)
    out[:, :k] = codes
    return out


# ---------------------------------------------------------------- 1: the product alone, codes made on the host
# (M, N, K): every M, N and K on both sides of the tile edges (32 rows in the few-rows form, 128 in the other), of the 16-byte pieces and
# of the 64-byte K step, and M on both sides of the switch between the forms.  WHICH form a row takes is asserted, not assumed:
# tests/test_qstatic_abi.py checks the table's coverage through th_debug_q8q8_plan (the host function the launch itself consumes).
PLAN_FIELDS = ("skinny", "tiles_m", "tiles_n", "grid")


def plan(B, K, N):
    out = (C.c_int * 4)()
    assert _lib().th_debug_q8q8_plan(B, K, N, C.cast(out, C.c_void_p)) == 0
    return dict(zip(PLAN_FIELDS, out))


CASES = [(1, 1, 1), (1, 10, 15), (1, 127, 16), (1, 128, 63), (1, 129, 64), (1, 300, 65), (1, 10, 784), (1, 300, 4112),
         (15, 1, 65), (15, 128, 784), (16, 10, 64), (16, 129, 16), (17, 127, 63), (17, 300, 1),
         (127, 1, 15), (127, 127, 784), (127, 300, 64),
         (128, 10, 4112), (128, 128, 64), (128, 128, 65), (128, 129, 16),
         (129, 1, 784), (129, 127, 1), (129, 129, 65), (129, 300, 63),
         (257, 1, 16), (257, 10, 15), (257, 127, 64), (257, 128, 784), (257, 129, 4112), (257, 300, 784),
         # the 32-row tiles of the few-rows form, and the last batch it takes
         (31, 129, 65), (32, 10, 784), (33, 127, 16), (64, 128, 63), (65, 300, 64), (256, 129, 65), (256, 10, 4112),
         # the 128 x 128 form: the first batch it takes, ragged and whole tiles
         (512, 129, 65), (513, 1, 16), (513, 128, 64), (513, 129, 65), (639, 300, 784), (640, 128, 4112), (640, 129, 15), (641, 10, 63), (641, 127, 1)]
PARAMS = [(1.0, (0.0, 1.0)), (0.0173, (-0.31, 0.0024))]      # (sx, {mw, sw}): pure integers (pins the lane maps), then a float codec
BPARAMS = (-0.27, 0.0019)


def test_case_table_crosses_every_edge():
    assert {c[0] for c in CASES} >= {1, 15, 16, 17, 127, 128, 129, 257}
    assert {c[1] for c in CASES} == {1, 10, 127, 128, 129, 300}
    assert {c[2] for c in CASES} == {1, 15, 16, 63, 64, 65, 784, 4112}
    assert len(set(CASES)) == len(CASES)
    assert {plan(*c[:1], c[2], c[1])["skinny"] for c in CASES} == {0, 1}      # both forms run (the edges of each: tests/test_qstatic_abi.py)


def _operands(M, N, K, seed):
    """int8 codes over the full range from two different generators, -128 and 127 in both where there is room"""
    rng = np.random.default_rng(seed)
    qx = rng.integers(-128, 128, (M, K)).astype(np.int8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    qw = ((n * 37 + k * 101 + (n * k) % 7 + rng.integers(0, 3, (N, K))) % 256 - 128).astype(np.int8)      # a skewed lattice, not qx's stream
    for q in (qx, qw):
        if q.size >= 2:
            q.reshape(-1)[0], q.reshape(-1)[-1] = -128, 127
    qb = rng.integers(-128, 128, N).astype(np.int8)
    return qx, qw, qb


def _product(ctx, qx, rs, sx, qw, wparams, qb, bparams, relu, pitch_x, pitch_w):
    """one th_linear_q8q8_fwd call: x padded with zeros, W's padding filled with a non-zero code (it must not matter), the output NaN-filled
    between two guard regions that must come back untouched, pool bytes in use unchanged"""
    (M, K), N = qx.shape, qw.shape[0]
    dx, dw = ctx.upload(_padded(qx, pitch_x).view(np.uint8)), ctx.upload(_padded(qw, pitch_w, 0x55).view(np.uint8))
    drs, dsx, dwp = ctx.upload(np.asarray(rs, np.int32)), ctx.upload(np.array([sx], f32)), ctx.upload(np.array(wparams, f32))
    db = ctx.upload(qb.view(np.uint8)) if qb is not None else None
    dbp = ctx.upload(np.array(bparams, f32)) if qb is not None else None
    ybuf = ctx.upload(np.full(M * N + 2 * GUARD, GUARD_BITS, np.uint32))
    y = ybuf.offset(4 * GUARD)
    ctx.call("th_fill_f32", y, float("nan"), M * N)
    before = _in_use(ctx)
    ctx.call("th_linear_q8q8_fwd", dx, pitch_x, drs, dsx, M, K, dw, pitch_w, N, dwp, db, dbp, relu, y)
    assert _in_use(ctx) == before
    out = ctx.download(ybuf, (M * N + 2 * GUARD,), np.uint32)
    assert (out[:GUARD] == GUARD_BITS).all() and (out[GUARD + M * N:] == GUARD_BITS).all(), "words around the output were written"
    return out[GUARD:GUARD + M * N].view(f32).reshape(M, N)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_product_is_the_reference_bit_for_bit(ctx, case):
    M, N, K = case
    i = CASES.index(case)
    qx, qw, qb = _operands(M, N, K, seed=M * 7919 + N * 31 + K)
    rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    pitch_x = _up16(K) + 16 * (i % 3)                       # the tightest pitch and looser ones
    pitch_w = -(-K // 64) * 64 if i % 2 else _up16(K)       # the twin's pitch (a multiple of the K step) and the tightest
    for (sx, wp), (bias, relu) in zip(PARAMS + PARAMS, ((0, 0), (1, 0), (1, 1), (0, 1))):
        ref = R.linear_q8q8(qx, sx, qw, wp, qb if bias else None, BPARAMS, relu)
        got = _product(ctx, qx, rs, sx, qw, wp, qb if bias else None, BPARAMS, relu, pitch_x, pitch_w)
        np.testing.assert_array_equal(_bits(got), _bits(ref), err_msg=str((case, sx, wp, "bias", bias, "relu", relu)))


def test_product_at_the_largest_k_with_the_extreme_codes(ctx):
    K = R.MAX_K
    qx = np.stack([np.full(K, -128, np.int8), np.full(K, 127, np.int8)])
    qw = np.stack([np.full(K, 127, np.int8), np.full(K, -128, np.int8), np.random.default_rng(1).integers(-128, 128, K).astype(np.int8)])
    rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    t, _ = R.int_terms(qx, qw)
    assert t.min() == -128 * 255 * K and t.max() == 127 * 255 * K      # the largest |t| there is: inside int32
    for sx, wp in PARAMS:
        got = _product(ctx, qx, rs, sx, qw, wp, None, None, 0, K, K)
        np.testing.assert_array_equal(_bits(got), _bits(R.linear_q8q8(qx, sx, qw, wp)))
    np.testing.assert_array_equal(_product(ctx, qx, rs, 1.0, qw, (0.0, 1.0), None, None, 0, K, K), t.astype(f32))


def test_identity_codes_return_the_asymmetric_weights_decoded(ctx):
    """A = I (code 1 on the diagonal, K = M, across a tile edge): y[m][n] = sw * (qw[n][m] + 128) + mw, the codec's decode of W transposed"""
    from oracle import train_extra as OX
    M = K = 130
    N = 70
    _, qw, _ = _operands(M, N, K, seed=5)
    assert not np.array_equal(qw[:, :N], qw[:, :N].T)
    qx = np.eye(M, dtype=np.int8)
    for wp in ((0.0, 1.0), (-0.31, 0.0024)):
        got = _product(ctx, qx, np.ones(M, np.int32), 1.0, qw, wp, None, None, 0, _up16(K), _up16(K))
        deq = OX.dequantize_int8(qw.reshape(-1), wp[1], -128, wp[0]).reshape(N, K)
        np.testing.assert_array_equal(_bits(got), _bits(deq.T))


# ---------------------------------------------------------------- 2: activations -> codes
def _quantize(ctx, x, dscale, pitch, xo=0):
    rows, k = x.shape
    raw = np.concatenate([np.zeros(xo, np.uint8), np.ascontiguousarray(x, f32).reshape(-1).view(np.uint8)])
    xbuf = ctx.upload(raw)
    dq, drs = ctx.upload(np.full(rows * pitch, 0x7F, np.uint8)), ctx.upload(np.full(rows, 0x7F7F7F7F, np.int32))
    before = _in_use(ctx)
    ctx.call("th_quantize_act_int8", xbuf.offset(xo), rows, k, dscale, dq, pitch, drs)
    assert _in_use(ctx) == before
    return ctx.download(dq, (rows, pitch), np.int8), ctx.download(drs, (rows,), np.int32)


@pytest.mark.parametrize("rows,k", [(1, 1), (3, 17), (64, 784), (5, 4112)])
def test_activation_codes_and_row_sums(ctx, rows, k):
    rng = np.random.default_rng(rows * 131 + k)
    x = (rng.standard_normal((rows, k)) * 2).astype(f32)
    if k >= 17:
        x[0, 3], x[rows - 1, 5], x[rows // 2, 16] = np.nan, np.inf, -np.inf      # (not finite: no part in the scale)
    # the tensor's own scale from th_fake_quant_act, and its output: codes * scale must be that output bit for bit
    dx, dy, dscale = ctx.upload(x), ctx.empty(rows * k), ctx.empty(1)
    ctx.call("th_fake_quant_act", dx, dy, rows * k, 0, dscale)
    scale = ctx.download(dscale, (1,))[0]
    assert _bits(scale) == _bits(R.act_scale_of(x))
    ref_q, ref_rs = R.quantize_act(x, scale)
    for pitch, xo in ((_up16(k), 0), (_up16(k) + 48, 0), (_up16(k), 4)):       # vector loads where k allows, a loose pitch, x off 16 bytes
        q, rs = _quantize(ctx, x, dscale, pitch, xo)
        np.testing.assert_array_equal(q[:, :k], ref_q)
        assert not q[:, k:].any(), "padding bytes must be 0"
        np.testing.assert_array_equal(rs, ref_rs)
        again = _quantize(ctx, x, dscale, pitch, xo)
        np.testing.assert_array_equal(q, again[0])
        np.testing.assert_array_equal(rs, again[1])
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(_bits(q[:, :k].astype(f32) * scale), _bits(ctx.download(dy, (rows, k))))
    if k >= 17:
        assert q[0, 3] == 0 and q[rows - 1, 5] == 127 and q[rows // 2, 16] == -128 and np.abs(q.astype(int)).max() >= 127


def test_a_row_of_the_lowest_code_at_the_largest_k(ctx):
    x = np.full((2, R.MAX_K), -1e9, f32)
    x[1] = 1e9
    q, rs = _quantize(ctx, x, ctx.upload(np.array([1.0], f32)), R.MAX_K)
    assert (q[0] == -128).all() and (q[1] == 127).all()
    assert rs[0] == -8388608 and rs[1] == 127 * R.MAX_K


def test_pad_rows(ctx):
    """k below, at and above a 16-byte piece and a pitch looser than the tight one; the packed source at an odd byte offset (its rows are not
    16-byte aligned in general), the destination between two guard regions that must come back untouched"""
    rng = np.random.default_rng(2)
    for rows, k, pitch in ((1, 1, 16), (7, 17, 64), (10, 784, 832), (3, 64, 64), (1, 15, 16), (2, 16, 16), (3, 17, 32), (5, 33, 96)):
        src = rng.integers(-128, 128, (rows, k)).astype(np.int8)
        n = rows * pitch
        sbuf = ctx.upload(np.concatenate([np.full(3, 0x33, np.uint8), src.reshape(-1).view(np.uint8), np.full(13, 0x33, np.uint8)]))
        dst = ctx.upload(np.concatenate([np.full(64, 0xA5, np.uint8), np.full(n, 0x7F, np.uint8), np.full(64, 0xA5, np.uint8)]))
        ctx.call("th_pad_rows_int8", sbuf.offset(3), rows, k, dst.offset(64), pitch)
        raw = ctx.download(dst, (n + 128,), np.uint8)
        assert (raw[:64] == 0xA5).all() and (raw[64 + n:] == 0xA5).all(), "bytes around the padded rows were written"
        np.testing.assert_array_equal(raw[64:64 + n].view(np.int8).reshape(rows, pitch), _padded(src, pitch))


# ---------------------------------------------------------------- 3: refusals (host checks before any launch)
def test_refusals_name_the_function_and_the_next_call_succeeds(ctx):
    hip = _lib()
    M, N, K = 3, 5, 32
    qx, qw, _ = _operands(M, N, K, seed=3)
    rs = qx.astype(np.int64).sum(axis=1).astype(np.int32)
    big = ctx.empty(70000 * 3 // 4 + 64, f32)
    dx, dw, drs = ctx.upload(qx.view(np.uint8)), ctx.upload(qw.view(np.uint8)), ctx.upload(rs)
    dsx, dwp, dy = ctx.upload(np.array([1.0], f32)), ctx.upload(np.array([0.0, 1.0], f32)), ctx.empty(M * N)

    def call(x=int(dx), px=K, k=K, w=int(dw), pw=K):
        return hip.th_linear_q8q8_fwd(ctx.h, x, px, int(drs), int(dsx), M, k, w, pw, N, int(dwp), None, None, 0, int(dy))

    before = _in_use(ctx)
    for what, kw in (("x off 16 bytes", dict(x=int(dx) + 4)), ("w off 16 bytes", dict(w=int(dw) + 8)), ("pitch_x % 16", dict(px=K + 8)),
                     ("pitch_w % 16", dict(pw=K + 4)), ("pitch below K", dict(px=16)),
                     ("in_features 65537", dict(x=int(big), w=int(big), k=65537, px=65552, pw=65552))):
        assert call(**kw) != 0 and b"th_linear_q8q8_fwd" in hip.th_last_error(), what
    assert hip.th_quantize_act_int8(ctx.h, int(dy), 1, 8, int(dsx), int(dx), 24, int(drs)) != 0 and b"th_quantize_act_int8" in hip.th_last_error()
    assert hip.th_pad_rows_int8(ctx.h, int(dx), 1, 8, int(dw), 24) != 0 and b"th_pad_rows_int8" in hip.th_last_error()
    assert _in_use(ctx) == before
    assert call() == 0
    np.testing.assert_array_equal(ctx.download(dy, (M, N)), R.linear_q8q8(qx, 1.0, qw, (0.0, 1.0)))


# ---------------------------------------------------------------- 4: the twin of an MLP
def _pool_in_use():
    import taper_amd as T
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


def _mlp(rng):
    import taper_amd as T
    model = T.Sequential([T.Linear(784, 128, True), T.ReLU(), T.Linear(128, 10, True)])
    vals = [(rng.standard_normal((128, 784)) / 28).astype(f32), (0.1 * rng.standard_normal(128)).astype(f32),
            (rng.standard_normal((10, 128)) / np.sqrt(128)).astype(f32), (0.1 * rng.standard_normal(10)).astype(f32)]
    for p, v in zip(model.parameters(), vals):
        p.set_data(v)
    return model, vals


def _ref_chain(ts, scales, x):
    """the reference forward of Linear + ReLU + Linear from the twin's packed tensors and activation scales"""
    (_, w1, p1), (_, b1, q1), (_, w2, p2), (_, b2, q2) = ts
    h = R.linear_q8q8(R.quantize_act(x, scales[0])[0], scales[0], w1.reshape(128, 784), p1, b1, q1, relu=True)
    return R.linear_q8q8(R.quantize_act(h, scales[1])[0], scales[1], w2.reshape(10, 128), p2, b2, q2)


@pytest.fixture(scope="module")
def mlp_twin():
    import taper_amd as T
    rng = np.random.default_rng(21)
    model, vals = _mlp(rng)
    calib = [rng.standard_normal((32, 784)).astype(f32), (2.5 * rng.standard_normal((32, 784))).astype(f32)]
    T.Tape.reset()
    q = model.quantize_static([T.Tensor(c, (32, 784)) for c in calib])
    return dict(model=model, vals=vals, calib=calib, q=q, tape_len=T.Tape.len(), ts=q.tensors(), scales=q.act_scales(), rng=rng)


def test_twin_scales_come_from_the_float_models_activations(mlp_twin):
    import taper_amd as T
    m, calib, scales = mlp_twin["model"], mlp_twin["calib"], mlp_twin["scales"]
    assert scales.dtype == f32 and scales.shape == (2,)
    assert _bits(scales[0]) == _bits(R.act_scale_of(*calib))      # the input's range is exact: min / max of the data
    assert np.abs(calib[1]).max() > np.abs(calib[0]).max() and scales[0] > R.act_scale_of(calib[0])      # the second tensor set it
    prefix = T.Sequential([m.layers[0], m.layers[1]])
    hidden = [prefix.forward(T.Tensor(c, (32, 784))).data() for c in calib]
    ref = R.act_scale_of(*hidden)
    assert abs(float(scales[1]) - float(ref)) <= RTOL * float(ref), (scales[1], ref)
    assert m.quantize("int8").act_scales().shape == (0,)


def test_twin_forward_is_the_reference_chain_bit_for_bit(mlp_twin):
    import taper_amd as T
    q, ts, scales = mlp_twin["q"], mlp_twin["ts"], mlp_twin["scales"]
    x = np.random.default_rng(22).standard_normal((37, 784)).astype(f32)
    T.Tape.reset()
    xt = T.Tensor(x, (37, 784)).requires_grad()
    before = _pool_in_use()
    y = q(xt)
    assert T.Tape.len() == 0 and y.tape_node() == 0
    got = y.data()
    del y
    assert _pool_in_use() == before      # codes, row sums and the hidden layer went back to the pool
    np.testing.assert_array_equal(_bits(got), _bits(_ref_chain(ts, scales, x)))
    for b in (0, 17, 36):
        alone = q(T.Tensor(x[b:b + 1], (1, 784))).data()
        np.testing.assert_array_equal(_bits(alone[0]), _bits(got[b]), err_msg=f"row {b} alone")
    # three times beyond the calibration range: the codes saturate, as the reference's do
    far = (3 * np.abs(mlp_twin["calib"][1]).max() * np.sign(x)).astype(f32)
    far[:, ::3] = x[:, ::3]
    assert np.abs(R.quantize_act(far, scales[0])[0].astype(int)).max() == 128
    np.testing.assert_array_equal(_bits(q(T.Tensor(far, (37, 784))).data()), _bits(_ref_chain(ts, scales, far)))


def test_twin_packs_what_the_weight_only_twin_packs_and_reads_only(mlp_twin):
    m, vals, q, ts = mlp_twin["model"], mlp_twin["vals"], mlp_twin["q"], mlp_twin["ts"]
    assert mlp_twin["tape_len"] == 0
    for p, v in zip(m.parameters(), vals):
        np.testing.assert_array_equal(_bits(p.data()), _bits(v))
    wo = m.quantize("int8")
    for (k1, c1, p1), (k2, c2, p2) in zip(ts, wo.tensors()):
        assert k1 == k2 == "int8"
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))
    step = _lib().th_qlinear_i8_kstep()
    padded = 128 * (-(-784 // step) * step) + 10 * (-(-128 // step) * step)
    assert q.storage_bytes() == padded + 128 + 10 + 8 * 4 + 4 * 2
    assert wo.storage_bytes() == 784 * 128 + 128 + 128 * 10 + 10 + 8 * 4


def test_all_zero_calibration_gives_the_unit_range():
    import taper_amd as T
    model, _ = _mlp(np.random.default_rng(23))
    for p in model.parameters()[:2]:
        p.set_data(np.zeros(p.numel(), f32))      # a first layer that outputs zeros: the second layer's calibration input is all zero too
    q = model.quantize_static(T.Tensor(np.zeros((4, 784), f32), (4, 784)))
    np.testing.assert_array_equal(_bits(q.act_scales()), _bits(np.array([1, 1], f32) / f32(127)))


def test_qat_layers_calibrate_and_deploy_as_their_inner_layers():
    """a QAT model with QAT switched on: the ranges are those of the plain float layers (no fake quantization in the calibration pass), the
    packed tensors those of the inner layers"""
    import taper_amd as T
    rng = np.random.default_rng(24)
    calib = T.Tensor(rng.standard_normal((16, 784)).astype(f32), (16, 784))
    plain = T.Sequential([T.Linear(784, 128, True, seed=3), T.ReLU(), T.Linear(128, 10, True, seed=4)])
    qat_model = T.Sequential([T.QATLinear(784, 128, True, seed=3), T.ReLU(), T.QATLinear(128, 10, True, seed=4)])
    for a, b in zip(plain.parameters(), qat_model.parameters()):
        np.testing.assert_array_equal(_bits(a.data()), _bits(b.data()))
    ref = plain.quantize_static(calib)
    T.qat.enable()
    try:
        T.Tape.reset()
        q = qat_model.quantize_static(calib)
        assert T.Tape.len() == 0
    finally:
        T.qat.disable()
    np.testing.assert_array_equal(_bits(q.act_scales()), _bits(ref.act_scales()))
    for (_, c1, p1), (_, c2, p2) in zip(q.tensors(), ref.tensors()):
        np.testing.assert_array_equal(c1, c2)
        np.testing.assert_array_equal(_bits(np.array(p1, f32)), _bits(np.array(p2, f32)))
    x = T.Tensor(rng.standard_normal((5, 784)).astype(f32), (5, 784))
    np.testing.assert_array_equal(_bits(q(x).data()), _bits(ref(x).data()))


# ---------------------------------------------------------------- 5: a conv model
def test_conv_front_runs_as_in_the_weight_only_twin():
    import taper_amd as T
    rng = np.random.default_rng(31)
    front = [T.Conv2dReLU(1, 4, (3, 3)), T.MaxPool2d((2, 2)), T.Flatten(1)]
    lin = T.Linear(4 * 5 * 5, 10, True)
    for p in front[0].parameters() + lin.parameters():
        p.set_data((0.3 * rng.standard_normal(p.numel())).astype(f32))
    model, prefix = T.Sequential(front + [lin]), T.Sequential(front)
    imgs = rng.uniform(0, 1, (8, 1, 12, 12)).astype(f32)
    calib = T.Tensor(rng.uniform(0, 1, (8, 1, 12, 12)).astype(f32), (8, 1, 12, 12))
    q = model.quantize_static(calib)
    feat = prefix.quantize("int8").forward(T.Tensor(imgs, imgs.shape)).data()      # the Linear's input: the weight-only twin of the same prefix
    assert feat.shape == (8, 100)
    scales, ts = q.act_scales(), q.tensors()
    assert scales.shape == (1,) and len(ts) == 4
    calib_feat = prefix.forward(calib).data()
    assert abs(float(scales[0]) - float(R.act_scale_of(calib_feat))) <= RTOL * float(scales[0])
    (_, w, wp), (_, b, bp) = ts[2:]
    ref = R.linear_q8q8(R.quantize_act(feat, scales[0])[0], scales[0], w.reshape(10, 100), wp, b, bp)
    np.testing.assert_array_equal(_bits(q(T.Tensor(imgs, imgs.shape)).data()), _bits(ref))


# ---------------------------------------------------------------- 6: refusals leak nothing
def test_static_refusals_leak_nothing():
    import taper_amd as T
    x = T.Tensor(np.zeros((2, 784), f32), (2, 784))
    dropout = T.Sequential([T.Linear(784, 128, True), T.ReLU(), T.Dropout(0.5), T.Linear(128, 10, True)])
    plain = T.Sequential([T.Linear(784, 128, True), T.ReLU(), T.Linear(128, 10, True)])
    wide = T.Sequential([T.Linear(65537, 2, True)])
    T.Device.sync()
    before = _pool_in_use()
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        dropout.quantize_static(x)
    with pytest.raises(T.TaperError, match="at least one calibration tensor"):
        plain.quantize_static([])
    with pytest.raises(T.TaperError, match="undefined calibration tensor"):
        plain.quantize_static([x, None])
    with pytest.raises(T.TaperError, match="65537"):
        wide.quantize_static(T.Tensor(np.zeros((1, 65537), f32), (1, 65537)))
    assert _pool_in_use() == before
    assert plain.quantize_static(x).act_scales().shape == (2,)      # and the next valid call succeeds


# ---------------------------------------------------------------- 7: accuracy, recorded only
def test_record_accuracy_against_the_float_model_and_the_weight_only_twin(mlp_twin):
    import taper_amd as T
    m, q = mlp_twin["model"], mlp_twin["q"]
    x = np.random.default_rng(41).standard_normal((256, 784)).astype(f32)
    xt = T.Tensor(x, (256, 784))
    got, fl, wo = q(xt).data(), m.forward(xt).data(), m.quantize("int8")(xt).data()
    # (the fixture's calibration set reaches 2.5 times further than these inputs; a twin calibrated on inputs like them beside it)
    matched = m.quantize_static(T.Tensor(np.random.default_rng(42).standard_normal((256, 784)).astype(f32), (256, 784)))(xt).data()
    T.Tape.reset()
    for name, a, ref in (("static_vs_float", got, fl), ("static_vs_weight_only", got, wo), ("static_matched_calibration_vs_float", matched, fl)):
        rec = margins.record("test_record_accuracy_against_the_float_model_and_the_weight_only_twin", name, a, ref)
        print(f"{name}: {rec['err_over_scale']:.3e} of max |y|")
