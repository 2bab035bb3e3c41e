"""The quantized Linear forward (csrc/qlinear.hip: th_linear_q8_fwd, th_linear_h16_fwd, th_dequantize_multi) against exact and
high-precision references, over every instance of the weight-streaming kernel (2 codecs x 4 batch tiles x vector / element loads x
one K slice / several) and the workspace path above th_qlinear_stream_max_batch() rows.

WHICH instance a row of the case table takes is asserted, not assumed: tests/test_quant_abi.py checks the table's coverage through
th_debug_qlinear_plan (the host function the launch itself consumes) without a GPU.

The exact-arithmetic checks rest on integers: x in [-4, 4], weights in [-128, 127] (int8 codes under {min_val = -128, scale = 1}, which
dequantize to themselves, or the half codes of those integers), biases in [-100, 100].  Every product and every partial sum is an integer
below 4 * 128 * K + 100 < 2^24 for K <= 8192, so every summation order on either path gives the integer result exactly."""
import ctypes as C

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle import train_extra as OX
from tests.test_gpu_quant import RTOL, _err
from tests.test_gpu_random_shapes import CFG

pytestmark = pytest.mark.gpu
f32 = np.float32

QT = {"int8": 0, "f16": 1}      # TH_QTYPE_INT8 / TH_QTYPE_F16
LOAD = {"int8": 16, "f16": 8}   # E: codes per 16-byte load
CODE = {"int8": 1, "f16": 2}    # bytes per code
PLAN_FIELDS = ("stream", "vec", "bt", "kslice", "S", "blocks_n", "want", "steps")


def _lib():
    from taper_amd._lib import hip
    return hip


def max_batch():
    return int(_lib().th_qlinear_stream_max_batch())


def plan(qtype, B, K, N, xo=0, wo=0):
    """th_debug_qlinear_plan as a dict (pure host code: no context, no device)"""
    out = (C.c_int * 8)()
    assert _lib().th_debug_qlinear_plan(QT[qtype], B, K, N, xo, wo, C.cast(out, C.c_void_p)) == 0
    return dict(zip(PLAN_FIELDS, out))


# (qtype, B, K, N, x offset, w offset): offsets in bytes off a 16-byte boundary.  tests/test_quant_abi.py asserts what this table covers.
CASES = [
    # ---- int8, vector loads (K % 16 == 0, aligned), one slice: bt 1 / 2 / 4 / 8
    ("int8", 1, 128, 10, 0, 0), ("int8", 2, 784, 128, 0, 0), ("int8", 3, 1024, 52, 0, 0), ("int8", 8, 512, 17, 0, 0),
    # ---- int8, vector loads, K split
    ("int8", 1, 2096, 10, 0, 0), ("int8", 2, 4096, 63, 0, 0), ("int8", 4, 3072, 5, 0, 0), ("int8", 7, 2064, 16, 0, 0),
    # ---- int8, element loads (ragged K), one slice -- K below one load among them
    ("int8", 1, 100, 52, 0, 0), ("int8", 2, 1000, 3, 0, 0), ("int8", 4, 15, 15, 0, 0), ("int8", 5, 1, 1, 0, 0),
    # ---- int8, element loads, K split: 2051 = 2 slices of 1024 and one of 3 elements
    ("int8", 1, 2051, 10, 0, 0), ("int8", 2, 1030, 2, 0, 0), ("int8", 3, 3000, 65, 0, 0), ("int8", 8, 2051, 17, 0, 0),
    # ---- f16, vector loads (K % 8 == 0), one slice
    ("f16", 1, 128, 10, 0, 0), ("f16", 2, 512, 128, 0, 0), ("f16", 4, 256, 52, 0, 0), ("f16", 8, 504, 17, 0, 0),
    # ---- f16, vector loads, K split
    ("f16", 1, 1048, 10, 0, 0), ("f16", 2, 2048, 63, 0, 0), ("f16", 3, 1536, 5, 0, 0), ("f16", 6, 1000, 16, 0, 0),
    # ---- f16, element loads, one slice
    ("f16", 1, 100, 52, 0, 0), ("f16", 2, 510, 3, 0, 0), ("f16", 4, 7, 15, 0, 0), ("f16", 8, 1, 1, 0, 0),
    # ---- f16, element loads, K split: 1027 = 2 slices of 512 and one of 3 elements
    ("f16", 1, 1027, 10, 0, 0), ("f16", 2, 515, 2, 0, 0), ("f16", 4, 1500, 65, 0, 0), ("f16", 5, 1027, 17, 0, 0),
    # ---- element loads by POINTER alone (K % E == 0): x off, w off, both; one slice and split
    ("int8", 1, 128, 10, 4, 0), ("int8", 3, 128, 10, 0, 1), ("int8", 8, 2048, 17, 12, 0), ("int8", 2, 2048, 17, 0, 7),
    ("int8", 4, 784, 5, 8, 15), ("f16", 1, 128, 10, 4, 0), ("f16", 3, 128, 10, 0, 2), ("f16", 8, 1024, 17, 8, 0),
    ("f16", 2, 1024, 17, 0, 14), ("f16", 4, 784, 5, 12, 6),
    # ---- ragged K on unaligned pointers
    ("int8", 2, 2051, 3, 4, 3), ("f16", 7, 1027, 3, 8, 10), ("int8", 8, 9, 2, 12, 5), ("f16", 1, 3, 5, 4, 2),
    # ---- fewer slices than asked for: 5 steps over 4 wanted slices -> 2 steps a slice, 3 slices
    ("int8", 1, 5120, 4096, 0, 0), ("f16", 2, 2560, 4096, 0, 0),
    # ---- N edges: one row, rows that re-read row N - 1, a second workgroup whose waves 1 to 3 return early, a ragged fifth
    ("int8", 3, 300, 1, 0, 0), ("int8", 1, 2051, 1, 0, 0), ("f16", 2, 300, 2, 0, 0), ("int8", 5, 300, 3, 0, 0), ("f16", 8, 300, 5, 0, 0),
    ("f16", 4, 1027, 15, 0, 0), ("int8", 2, 300, 16, 0, 0), ("f16", 3, 300, 17, 0, 0), ("int8", 8, 300, 63, 0, 0), ("f16", 1, 300, 65, 0, 0),
    # ---- so many rows that no split is asked for: several K steps in one slice
    ("int8", 2, 3000, 16384, 0, 0), ("f16", 1, 1536, 16400, 0, 0),
    # ---- the workspace path: max + 1 rows and 17
    ("int8", 9, 2051, 10, 0, 0), ("f16", 9, 1027, 10, 0, 0), ("int8", 17, 784, 128, 0, 0), ("f16", 17, 100, 52, 0, 0),
    ("int8", 9, 128, 17, 4, 1), ("f16", 17, 515, 3, 8, 2), ("int8", 17, 5120, 4096, 0, 0), ("f16", 9, 1, 1, 0, 0),
]


def _id(c):
    return "-".join(str(v) for v in c)


GUARD = 64                 # words on either side of an output
GUARD_BITS = 0xFFA5C3E1    # a NaN payload no computation produces (th_fill_f32's NaN is 0x7FC00000)


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


def _place(ctx, a, off=0):
    """`a` in device memory, `off` bytes past a 16-byte boundary -> (the allocation, kept alive by the caller; the pointer)"""
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = ctx.upload(np.concatenate([np.zeros(off, np.uint8), raw, np.zeros(4, np.uint8)]))
    assert int(buf) % 16 == 0
    return buf, buf.offset(off)


def _codes(qtype, w):
    """integers in [-128, 127] as codes that dequantize to themselves: int8 under {min_val = -128, scale = 1}, or their half codes"""
    w = np.asarray(w)
    assert w.min() >= -128 and w.max() <= 127
    return w.astype(np.int8) if qtype == "int8" else OX.f32_to_f16_bits(np.arange(-128, 128).astype(f32))[w + 128]


class Layer:
    """one quantized Linear's operands on the device: codes (any shape [N, K]), params (int8), bias codes / params (nullable)"""

    def __init__(self, ctx, qtype, wcodes, wparams=None, bcodes=None, bparams=None, wo=0):
        self.ctx, self.qtype = ctx, qtype
        self.N, self.K = wcodes.shape
        self.keep = []
        self.w = self._put(wcodes, wo)
        self.wp = self._put(np.asarray(wparams, f32)) if qtype == "int8" else None
        self.b = self._put(bcodes) if bcodes is not None else None
        self.bp = self._put(np.asarray(bparams, f32)) if (qtype == "int8" and bcodes is not None) else None

    def _put(self, a, off=0):
        buf, ptr = _place(self.ctx, a, off)
        self.keep.append(buf)
        return ptr

    def put_x(self, x, xo=0):
        buf, ptr = _place(self.ctx, np.asarray(x, f32), xo)
        return buf, ptr

    def call(self, xptr, B, relu, bias, y):
        if self.qtype == "int8":
            self.ctx.call("th_linear_q8_fwd", xptr, B, self.K, self.w, self.N, self.wp, self.b if bias else None, self.bp if bias else None,
                          relu, y)
        else:
            self.ctx.call("th_linear_h16_fwd", xptr, B, self.K, self.w, self.N, self.b if bias else None, relu, y)

    def forward(self, x, xo=0, relu=0, bias=False):
        """y [B, N] of one call: the output NaN-filled between two guard regions that must come back untouched, pool bytes in use
        the same before and after (the partials buffer and the dequantize workspace went back)"""
        ctx, B = self.ctx, x.shape[0]
        n = B * self.N
        xbuf, xptr = self.put_x(x, xo)
        ybuf = ctx.upload(np.full(n + 2 * GUARD, GUARD_BITS, np.uint32))
        y = ybuf.offset(4 * GUARD)
        ctx.call("th_fill_f32", y, float("nan"), n)
        before = _in_use(ctx)
        self.call(xptr, B, relu, bias, y)
        assert _in_use(ctx) == before, "pool bytes in use changed over the call"
        out = ctx.download(ybuf, (n + 2 * GUARD,), np.uint32)
        assert (out[:GUARD] == GUARD_BITS).all(), "the words before the output were written"
        assert (out[GUARD + n:] == GUARD_BITS).all(), "the words after the output were written"
        del xbuf
        return out[GUARD:GUARD + n].view(f32).reshape(B, self.N)


def _same_values(got, ref, msg=""):
    """bit equality with +0 == -0 (no NaN on either side)"""
    assert not np.isnan(got).any(), msg
    np.testing.assert_array_equal(got, ref, err_msg=str(msg))


# ---------------------------------------------------------------- exact arithmetic
def _exact(ctx, qtype, B, K, N, xo, wo, seed, combos=((0, 0), (0, 1), (1, 0), (1, 1))):
    assert 4 * 128 * K + 100 < 2 ** 24
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (B, K))
    w = rng.integers(-128, 128, (N, K))
    b = rng.integers(-100, 101, N)
    one = [-128.0, 1.0]   # {min_val, scale}: (q + 128) * 1 + (-128) == q exactly
    layer = Layer(ctx, qtype, _codes(qtype, w).reshape(N, K), one, _codes(qtype, b), one, wo)
    prod = x.astype(np.int64) @ w.T.astype(np.int64)
    for relu, bias in combos:
        ref = prod + b[None, :] if bias else prod
        ref = np.maximum(ref, 0) if relu else ref
        got = layer.forward(x.astype(f32), xo, relu, bool(bias))
        _same_values(got, ref.astype(f32), (qtype, B, K, N, xo, wo, "relu", relu, "bias", bias))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_integer_data_is_exact_on_every_form(ctx, case):
    qtype, B, K, N, xo, wo = case
    _exact(ctx, qtype, B, K, N, xo, wo, seed=B * 7919 + K * 31 + N * 3 + xo + wo)


@settings(**CFG)
@given(qtype=st.sampled_from(["int8", "f16"]), B=st.integers(1, 2 * max_batch() + 1), K=st.integers(1, 3000), N=st.integers(1, 70), bias=st.integers(0, 1),
       relu=st.integers(0, 1), xo=st.sampled_from([0, 4, 8, 12]), wo=st.integers(0, 7))
def test_drawn_shapes_are_exact(ctx, qtype, B, K, N, bias, relu, xo, wo):
    _exact(ctx, qtype, B, K, N, xo, wo * CODE[qtype], seed=K * 71 + N, combos=((relu, bias),))


# ---------------------------------------------------------------- float data
def _float_layer(ctx, qtype, K, N, rng, wo=0):
    """He-scaled weights through the codecs -> (Layer, dequantized W [N, K] f32, dequantized b [N] f32, the code arrays for a twin)"""
    s = np.sqrt(2.0 / K)
    w = rng.uniform(-s, s, (N, K)).astype(f32)
    b = rng.uniform(-0.1, 0.1, N).astype(f32)
    if qtype == "int8":
        qw, ws, _, wm = OX.quantize_int8(w)
        qb, bs, _, bm = OX.quantize_int8(b)
        wdeq, bdeq = OX.dequantize_int8(qw, ws, -128, wm).reshape(N, K), OX.dequantize_int8(qb, bs, -128, bm)
        args = (qw.reshape(N, K), [wm, ws], qb, [bm, bs])
    else:
        hw, hb = OX.f32_to_f16_bits(w), OX.f32_to_f16_bits(b)
        wdeq, bdeq = _half_table()[hw].reshape(N, K), _half_table()[hb]
        args = (hw.reshape(N, K), None, hb, None)
    return Layer(ctx, qtype, *args, wo), wdeq, bdeq, args


_HALF = []


def _half_table():
    """the oracle's decode of all 65 536 half codes"""
    if not _HALF:
        _HALF.append(OX.f16_bits_to_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16)))
    return _HALF[0]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# (thinned: the two 16 384-row layers stay with the exact test -- their codecs on the host cost more than every other row together)
FLOAT_CASES = [c for c in CASES if c[2] * c[3] <= 1 << 25]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=_id)
def test_float_data_parity_and_structural_identities(ctx, case):
    """The project's parity (RTOL on the _err metric) against the float64 product of the dequantized weights, and what the kernel's
    structure gives bit for bit: the accumulation order depends on K and N only and each (weight row, batch row) accumulator is its own
    fmaf chain (-ffp-contract=off, no fast-math), so (a) on the streaming path row b of a B-row call equals the same row sent alone,
    whichever batch tile either call takes, and (b) for K % E == 0 the element-load instance (x or W off a 16-byte boundary) equals
    the vector-load instance on the same data, +0 and -0 taken as equal."""
    qtype, B, K, N, xo, wo = case
    big = K * N > (1 << 22)
    rng = np.random.default_rng(B * 7919 + K * 31 + N)
    layer, wdeq, bdeq, args = _float_layer(ctx, qtype, K, N, rng, wo)
    x = rng.standard_normal((B, K)).astype(f32)
    prod = x.astype(np.float64) @ wdeq.astype(np.float64).T
    outs = {}
    for relu, bias in ((0, 1),) if big else ((0, 0), (0, 1), (1, 0), (1, 1)):
        ref = prod + bdeq.astype(np.float64)[None, :] if bias else prod
        ref = np.maximum(ref, 0) if relu else ref
        got = outs[relu, bias] = layer.forward(x, xo, relu, bool(bias))
        assert np.isfinite(got).all()
        e = _err(got, ref)
        print(f"float parity {case} relu={relu} bias={bias}: err {e:.3e}")
        assert e <= RTOL, (relu, bias, e)
    streaming = plan(qtype, B, K, N, xo, wo)["stream"] == 1
    if streaming and B > 1:
        for b in range(B):
            alone = layer.forward(x[b:b + 1], xo, 0, True)
            np.testing.assert_array_equal(_bits(alone[0]), _bits(outs[0, 1][b]), err_msg=f"row {b} alone")
    if streaming and K % LOAD[qtype] == 0:
        forms = {}
        for o in ((0, 0), (4, 0), (0, CODE[qtype]), (12, 16 - CODE[qtype])):
            twin = layer if o[1] == wo else Layer(ctx, qtype, *args, o[1])
            assert plan(qtype, B, K, N, *o)["vec"] == (o == (0, 0))
            forms[o] = twin.forward(x, o[0], 0, True)
        for o, got in forms.items():
            _same_values(got, forms[0, 0], f"offsets {o} against the aligned call")


# ---------------------------------------------------------------- decode mapping
def _onehot_ks(qtype, K, N):
    """k positions that land in every byte / half of a word and every word of a load (first lane, first step), the last lane of the
    first step, the first and last lane of the last step, the first and last element of every slice, and the last element of K"""
    E, p = LOAD[qtype], plan(qtype, 1, K, N)
    ks = set(range(E)) | {63 * E + j for j in (0, E - 1)} | {K - 1, 0}
    for s in range(p["S"]):
        lo, hi = s * p["kslice"], min(K, (s + 1) * p["kslice"])
        ks |= {lo, lo + 1, hi - 1, lo + 64 * E - 1, hi - E, max(lo, hi - 64 * E), max(lo, hi - 64 * E) + E - 1}
    last_step = (p["steps"] - 1) * 64 * E
    ks |= {last_step, last_step + 63 * E, K - 2}
    return sorted(k for k in ks if 0 <= k < K)


@pytest.mark.parametrize("qtype", ["int8", "f16"])
@pytest.mark.parametrize("form", ["vec_split", "ragged_split", "one_load", "vec_one_slice", "ragged_offsets"])
def test_one_hot_rows_read_back_the_decoded_weight(ctx, qtype, form):
    """x row b is the unit vector at k_b: y[b, n] must be deq(W[n, k_b]) (+ deq(bias[n]), one f32 rounding) bit for bit -- which
    byte of which word of which lane's load of which step of which slice feeds which k.  int8 carries real params and the codes
    -128, -1, 0 and 127; both paths (chunks of up to max rows through the streaming kernel, all rows at once through the workspace)."""
    E = LOAD[qtype]
    K, N, xo, wo = {"vec_split": (3 * 64 * E, 10, 0, 0), "ragged_split": (2 * 64 * E + E + 3, 10, 0, 0), "one_load": (E + 3, 5, 0, 0),
                    "vec_one_slice": (64 * E, 17, 0, 0), "ragged_offsets": (2 * 64 * E + 3, 3, 4, 3 * CODE[qtype])}[form]
    rng = np.random.default_rng(K + N)
    w = rng.uniform(-1, 1, (N, K)).astype(f32)
    b = rng.uniform(-0.5, 0.5, N).astype(f32)
    ks = _onehot_ks(qtype, K, N)
    if qtype == "int8":
        qw, ws, _, wm = OX.quantize_int8(w)
        qb, bs, _, bm = OX.quantize_int8(b)
        qw = qw.reshape(N, K).copy()
        for i, k in enumerate(ks):               # the extreme codes and the sign bit, at the probed positions
            qw[i % N, k] = (-128, -1, 0, 127)[i % 4]
            qw[(i + 1) % N, k] = (127, -128, -1, 0)[i % 4]
        wdeq, bdeq = OX.dequantize_int8(qw, ws, -128, wm).reshape(N, K), OX.dequantize_int8(qb, bs, -128, bm)
        layer = Layer(ctx, qtype, qw, [wm, ws], qb, [bm, bs], wo)
    else:
        hw, hb = OX.f32_to_f16_bits(w).reshape(N, K), OX.f32_to_f16_bits(b)
        wdeq, bdeq = OX.f16_bits_to_f32(hw).reshape(N, K), OX.f16_bits_to_f32(hb)
        layer = Layer(ctx, qtype, hw, None, hb, None, wo)
    assert np.isfinite(wdeq).all()
    M = max_batch()
    chunks = [ks[i:i + M] for i in range(0, len(ks), M)] + [ks[:1], ks[-2:], ks[:3], ks]
    assert len(ks) > M and plan(qtype, len(ks), K, N, xo, wo)["stream"] == 0
    for chunk in chunks:
        x = np.zeros((len(chunk), K), f32)
        x[np.arange(len(chunk)), chunk] = 1
        for bias in (False, True):
            ref = wdeq[:, chunk].T.astype(f32)
            ref = (ref + bdeq[None, :].astype(f32)).astype(f32) if bias else ref
            got = layer.forward(x, xo, 0, bias)
            _same_values(got, ref, (qtype, form, "k", chunk, "bias", bias))


# ---------------------------------------------------------------- special values
H_PINF, H_NINF, H_NAN, H_SUB_MIN, H_SUB_MAX, H_NZERO = 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x03FF, 0x8000


def _ieee_product(x, w):
    """float64 x . w^T term by term under numpy's IEEE rules (no BLAS: inf * 0 and NaN must propagate)"""
    with np.errstate(all="ignore"):
        return (x.astype(np.float64)[:, None, :] * w.astype(np.float64)[None, :, :]).sum(axis=-1)


def _special_x(rng, B, K):
    """normal rows; row 1 holds a NaN, row 2 +inf and -inf (the last element of K among them), row 3 exact zeros throughout"""
    x = rng.standard_normal((B, K)).astype(f32)
    special = np.zeros(B, bool)
    if B > 1:
        x[1, min(3, K - 1)] = np.nan
    if B > 2:
        x[2, min(7, K - 2)] = np.inf
        x[2, K - 1] = -np.inf
    if B > 3:
        x[3, :] = 0
    special[1:4] = True
    return x, special


def _check_special(got, pre, relu, tag):
    """classes where the reference is NaN / +inf / -inf, RTOL on the finite rest; with ReLU a NaN pre-activation gives +0"""
    with np.errstate(all="ignore"):
        ref = np.where(np.isnan(pre), 0.0, np.maximum(pre, 0)) if relu else pre
    nan, pinf, ninf = np.isnan(ref), ref == np.inf, ref == -np.inf
    assert (np.isnan(got) == nan).all(), (tag, "NaN class")
    assert ((got == np.inf) == pinf).all() and ((got == -np.inf) == ninf).all(), (tag, "inf class")
    fin = ~(nan | pinf | ninf)
    if relu:
        dead = np.isnan(pre) | (pre == -np.inf)
        assert (_bits(got)[dead] == 0).all(), (tag, "ReLU of NaN / -inf is +0")
    if fin.any():
        e = _err(got[fin], ref[fin])
        assert e <= RTOL, (tag, e)


def _special_batches():
    M = max_batch()
    return list(range(1, M + 1)) + [M + 1]


@pytest.mark.parametrize("K,N,xo,wo", [(1027, 13, 0, 0), (1032, 13, 0, 0), (1024, 6, 4, 2), (11, 3, 0, 0)])
def test_f16_special_codes_and_special_x(ctx, K, N, xo, wo):
    """+-inf, NaN, the smallest and the largest subnormal and -0 as weight codes -- inside rows, at row ends and in the last, partly
    filled load -- with NaN, +-inf and exact zeros in x on some batch rows: the output has the class of the float64 IEEE product
    wherever that is NaN or infinite and holds RTOL elsewhere; rows of x and of W that hold nothing special equal, bit for bit, the
    same call with the special entries replaced by zeros (nothing leaks from a neighbour's accumulator, pad element or slice).
    Finite magnitudes stay near 1, so f32 cannot overflow where float64 does not."""
    rng = np.random.default_rng(K * 13 + N)
    s = np.sqrt(2.0 / K)
    hw = OX.f32_to_f16_bits(rng.uniform(-s, s, (N, K)).astype(f32)).reshape(N, K)
    hb = OX.f32_to_f16_bits(rng.uniform(-0.1, 0.1, N).astype(f32))
    hw[0, 0], hw[0, K // 2], hw[0, K - 1] = H_SUB_MIN, H_NZERO, H_SUB_MAX             # finite specials: row 0 stays finite
    hw[1, 5 % K], hw[1, K - 1] = H_PINF, H_NZERO
    hw[2, 0], hw[2, K - 2] = H_NINF, H_SUB_MAX
    if N > 4:
        hw[4, K - 1] = H_NAN                                                          # the last, partly filled load
        hw[5, 3], hw[5, K - 3] = H_PINF, H_NINF                                       # inf - inf within one row
    if N > 12:
        hw[N - 1, K - 2] = H_PINF                                                     # the last row, whose wave re-reads it for rows past N
        hw[N - 2, K // 2 + 1] = H_NAN
    wspecial = ~np.isfinite(_half_table()[hw]).all(axis=1)
    assert wspecial.any() and not wspecial.all()
    layer, clean = Layer(ctx, "f16", hw, None, hb, None, wo), Layer(ctx, "f16", np.where(np.isfinite(_half_table()[hw]), hw, 0).astype(np.uint16),
                                                                    None, hb, None, wo)
    wdeq, bdeq = _half_table()[hw], _half_table()[hb].astype(np.float64)
    for B in _special_batches():
        x, xspecial = _special_x(rng, B, K)
        x0 = np.where(np.isfinite(x), x, 0).astype(f32)
        with np.errstate(all="ignore"):
            pre = _ieee_product(x, wdeq) + bdeq[None, :]
        for relu in (0, 1):
            got = layer.forward(x, xo, relu, True)
            _check_special(got, pre, relu, (K, N, B, relu))
            twin = clean.forward(x0, xo, relu, True)
            keep = np.ix_(~xspecial, ~wspecial)
            np.testing.assert_array_equal(_bits(got[keep]), _bits(twin[keep]), err_msg=f"clean rows changed: B={B} relu={relu}")


@pytest.mark.parametrize("K,N,xo,wo", [(2051, 13, 0, 0), (2048, 5, 0, 0), (19, 3, 4, 1)])
def test_int8_weights_with_special_x(ctx, K, N, xo, wo):
    """NaN, +-inf and exact zeros in x over int8 weights (finite by construction): classes, RTOL and untouched neighbours as above"""
    rng = np.random.default_rng(K * 17 + N)
    layer, wdeq, bdeq, _ = _float_layer(ctx, "int8", K, N, rng, wo)
    for B in _special_batches():
        x, xspecial = _special_x(rng, B, K)
        x0 = np.where(np.isfinite(x), x, 0).astype(f32)
        with np.errstate(all="ignore"):
            pre = _ieee_product(x, wdeq) + bdeq.astype(np.float64)[None, :]
        for relu in (0, 1):
            got = layer.forward(x, xo, relu, True)
            _check_special(got, pre, relu, (K, N, B, relu))
            twin = layer.forward(x0, xo, relu, True)
            np.testing.assert_array_equal(_bits(got[~xspecial]), _bits(twin[~xspecial]), err_msg=f"clean rows changed: B={B} relu={relu}")


# ---------------------------------------------------------------- th_dequantize_multi
def _dq_items(ctx, specs, rng):
    """specs: [(qtype, n)] -> (ctypes array, [(out allocation, n, reference f32 or None)], keepalive)"""
    from taper_amd import hip as H
    items, outs, keep = (H.QTensor * len(specs))(), [], []
    for i, (qtype, n) in enumerate(specs):
        if n == 0:
            items[i] = H.QTensor(None, None, None, 0, QT[qtype])   # (null pointers: nothing is read or written)
            outs.append((None, 0, None))
            continue
        if qtype == "int8":
            codes = rng.integers(-128, 128, n).astype(np.int8)
            mn, scale = f32(rng.uniform(-3, 0)), f32(rng.uniform(1e-3, 0.05))
            ref = OX.dequantize_int8(codes, scale, -128, mn)
            params = ctx.upload(np.array([mn, scale], f32))
        else:
            codes = rng.integers(0, 65536, n).astype(np.uint16)
            ref, params = _half_table()[codes], None
        dc = ctx.upload(codes.view(np.uint8) if qtype == "int8" else codes)
        out = ctx.upload(np.full(n + GUARD, GUARD_BITS, np.uint32))
        keep += [dc, params]
        items[i] = H.QTensor(int(dc), int(params) if params is not None else None, int(out), n, QT[qtype])
        outs.append((out, n, ref))
    return items, outs, keep


def _dq_check(ctx, outs):
    for i, (out, n, ref) in enumerate(outs):
        if not n:
            continue
        got = ctx.download(out, (n + GUARD,), np.uint32)
        assert (got[n:] == GUARD_BITS).all(), f"item {i}: the words after the output were written"
        nan = np.isnan(ref)                       # NaN compares as NaN of any payload (the observers' rule)
        assert (np.isnan(got[:n].view(f32)) == nan).all(), i
        np.testing.assert_array_equal(got[:n][~nan], _bits(ref)[~nan], err_msg=f"item {i}")


@pytest.mark.parametrize("n_items", [33, 64, 65])
def test_dequantize_multi_chunks_of_32(ctx, n_items):
    """lists that end a chunk of 32 exactly or spill one item into the next launch: mixed codecs, lengths around the 256-thread
    workgroup and one long odd one, zero-length items (null pointers) first, in the middle and last"""
    rng = np.random.default_rng(n_items)
    lens = [1, 3, 255, 257, 100003, 0]
    specs = [("int8" if (i * 7 + i // 3) % 2 else "f16", lens[i % len(lens)]) for i in range(n_items)]
    for i in (0, n_items // 2, 31, 32, n_items - 1):
        specs[i] = (specs[i][0], 0)
    assert {n for _, n in specs} == set(lens) and {q for q, _ in specs} == {"int8", "f16"}
    items, outs, keep = _dq_items(ctx, specs, rng)
    before = _in_use(ctx)
    ctx.call("th_dequantize_multi", C.addressof(items), n_items)
    assert _in_use(ctx) == before
    _dq_check(ctx, outs)


def test_dequantize_multi_every_half_code(ctx):
    from taper_amd import hip as H
    codes = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    dc, out = ctx.upload(codes), ctx.upload(np.full(65536 + GUARD, GUARD_BITS, np.uint32))
    items = (H.QTensor * 1)(H.QTensor(int(dc), None, int(out), 65536, 1))
    ctx.call("th_dequantize_multi", C.addressof(items), 1)
    _dq_check(ctx, [(out, 65536, _half_table())])
    got = ctx.download(out, (65536,), np.uint32)
    nan = np.isnan(_half_table())
    assert nan.sum() == 2 * 1023
    np.testing.assert_array_equal(got[nan] >> 31, codes[nan] >> 15)   # (a NaN keeps its sign, whatever its payload)


def test_dequantize_multi_large_items_and_the_grid_cap(ctx):
    """one 4096 x 4096 tensor alone (the element-wise grid cap and the grid-stride walk), and 32 items of which one is very large
    (2048 / 32 = 64 workgroups an item: the large one walks 256 strides, the small ones leave most workgroups idle)"""
    rng = np.random.default_rng(5)
    for specs in ([("int8", 4096 * 4096)], [("f16" if i % 2 else "int8", (1 << 22) + 3 if i == 13 else (0 if i == 20 else 1 + 37 * i)) for i in range(32)]):
        items, outs, keep = _dq_items(ctx, specs, rng)
        ctx.call("th_dequantize_multi", C.addressof(items), len(specs))
        _dq_check(ctx, outs)
        del items, outs, keep


# ---------------------------------------------------------------- refusals
def _refused(ctx, rc, entry):
    msg = _lib().th_last_error().decode()
    assert rc != 0 and entry in msg, (rc, msg)


def test_linear_refusals_name_their_entry_point_and_touch_nothing(ctx):
    """every TH_REQUIRE of qlinear_fwd: nonzero, a message naming the entry point, the NaN-filled output untouched, pool bytes in
    use unchanged, and the context usable afterwards.  B == 0 returns 0 and writes nothing."""
    L = _lib()
    K, N, B = 100, 7, 2
    rng = np.random.default_rng(0)
    x = ctx.upload(rng.standard_normal((B, K)).astype(f32))
    w8, b8 = ctx.upload(rng.integers(0, 256, N * K).astype(np.uint8)), ctx.upload(rng.integers(0, 256, N).astype(np.uint8))
    w16, b16 = ctx.upload(rng.integers(0, 0x3C00, N * K).astype(np.uint16)), ctx.upload(rng.integers(0, 0x3C00, N).astype(np.uint16))
    p = ctx.upload(np.array([-1.0, 0.01], f32))
    y = ctx.empty(B * N)
    ctx.call("th_fill_f32", y, float("nan"), B * N)
    X, W8, B8, W16, B16, P, Y = (int(v) for v in (x, w8, b8, w16, b16, p, y))
    before = _in_use(ctx)

    def q8(x=X, B=B, K=K, w=W8, N=N, wp=P, b=B8, bp=P, y=Y):
        return L.th_linear_q8_fwd(ctx.h, x, B, K, w, N, wp, b, bp, 0, y)

    def h16(x=X, B=B, K=K, w=W16, N=N, b=B16, y=Y):
        return L.th_linear_h16_fwd(ctx.h, x, B, K, w, N, b, 1, y)

    for fn, entry in ((q8, "th_linear_q8_fwd"), (h16, "th_linear_h16_fwd")):
        for bad in (dict(K=0), dict(K=-3), dict(N=0), dict(N=-1), dict(B=-1), dict(x=None), dict(w=None), dict(y=None)):
            _refused(ctx, fn(**bad), entry)
        assert fn(B=0) == 0                                   # nothing to do: no launch, nothing written
        assert fn(B=0, b=None) == 0
    _refused(ctx, q8(wp=None), "th_linear_q8_fwd")            # int8 without wparams
    _refused(ctx, q8(bp=None), "th_linear_q8_fwd")            # int8 bias codes without bparams
    _refused(ctx, q8(B=17, bp=None), "th_linear_q8_fwd")      # (the same on the workspace path's batch)
    _refused(ctx, h16(B=17, w=None), "th_linear_h16_fwd")
    assert _in_use(ctx) == before
    assert np.isnan(ctx.download(y, (B * N,))).all(), "a refused (or B == 0) call wrote to its output"
    assert q8() == 0 and np.isfinite(ctx.download(y, (B * N,))).all()          # the context is still usable
    assert h16() == 0 and np.isfinite(ctx.download(y, (B * N,))).all()
    _exact(ctx, "int8", 3, 100, 7, 0, 0, seed=1)
    _exact(ctx, "f16", 9, 100, 7, 0, 0, seed=2)


def test_dequantize_multi_refusals(ctx):
    """a bad qtype, a negative length, and n > 0 with null codes, null out or (int8) null params: refused before anything is
    launched -- the good item ahead of the bad one in the list keeps its NaN fill"""
    from taper_amd import hip as H
    L = _lib()
    n = 300
    c8, c16 = ctx.upload(np.arange(n, dtype=np.uint8)), ctx.upload(np.arange(n, dtype=np.uint16))
    p = ctx.upload(np.array([-1.0, 0.01], f32))
    o1, o2 = ctx.empty(n), ctx.empty(n)
    for o in (o1, o2):
        ctx.call("th_fill_f32", o, float("nan"), n)
    good = H.QTensor(int(c16), None, int(o1), n, 1)
    before = _in_use(ctx)
    for bad in (H.QTensor(int(c8), int(p), int(o2), n, 2), H.QTensor(int(c8), int(p), int(o2), n, -1), H.QTensor(int(c8), int(p), int(o2), -1, 0),
                H.QTensor(None, int(p), int(o2), n, 0), H.QTensor(int(c8), int(p), None, n, 0), H.QTensor(int(c8), None, int(o2), n, 0),
                H.QTensor(None, None, int(o2), n, 1), H.QTensor(int(c16), None, None, n, 1)):
        items = (H.QTensor * 2)(good, bad)
        _refused(ctx, L.th_dequantize_multi(ctx.h, C.addressof(items), 2), "th_dequantize_multi")
    items = (H.QTensor * 2)(good, good)
    _refused(ctx, L.th_dequantize_multi(ctx.h, None, 2), "th_dequantize_multi")
    _refused(ctx, L.th_dequantize_multi(ctx.h, C.addressof(items), -1), "th_dequantize_multi")
    assert L.th_dequantize_multi(ctx.h, None, 0) == 0
    assert _in_use(ctx) == before
    for o in (o1, o2):
        assert np.isnan(ctx.download(o, (n,))).all(), "a refused list wrote to an output"
    ok = (H.QTensor * 2)(good, H.QTensor(int(c8), int(p), int(o2), n, 0))      # the context is still usable
    assert L.th_dequantize_multi(ctx.h, C.addressof(ok), 2) == 0
    np.testing.assert_array_equal(_bits(ctx.download(o1, (n,))), _bits(_half_table()[np.arange(n)]))
    np.testing.assert_array_equal(_bits(ctx.download(o2, (n,))), _bits(OX.dequantize_int8(np.arange(n).astype(np.uint8).view(np.int8), 0.01, -128, -1.0)))
