"""Numpy restatement of calibrated int8 inference (csrc/qgemm_i8.hip), exact to the bit:

    qx  = clamp(round(x / sx) as i32, -128, 127)            th_fake_quant_act's int8 code (NaN -> 0, +-inf saturate)
    acc = sum_k qx[b][k] * qw[n][k],  rs = sum_k qx[b][k],  t = acc + 128 * rs          int32, exact
    y   = sx * (sw * (float)t + mw * (float)rs)  [+ dequantize_int8(qb[n])]  [max(y, 0)]   f32, every operation rounded once

The rounding idiom is fq_act_int8's of tests/test_gpu_qat.py; the weight codecs are oracle.train_extra's."""
import numpy as np

from oracle import train_extra as OX

f32 = np.float32
MAX_K = 65536


def act_scale(mn, mx):
    """the scale th_fake_quant_act gives the finite range [mn, mx] (fake_quantize.rs:94-118: all zero -> (0, 1), all equal -> +-10 %)"""
    mn, mx = f32(mn), f32(mx)
    if mn == mx:
        mn, mx = (f32(0), f32(1)) if mn == 0 else (f32(mn * f32(0.9)), f32(mn * f32(1.1)))
    return f32(max(abs(mn), abs(mx)) / f32(127))


def act_scale_of(*tensors):
    """act_scale of the finite min / max over every tensor of a calibration set"""
    fin = np.concatenate([np.asarray(t, f32).reshape(-1) for t in tensors])
    fin = fin[np.isfinite(fin)]
    mn, mx = (f32(fin.min()), f32(fin.max())) if fin.size else (f32(np.inf), f32(-np.inf))
    return act_scale(mn, mx)


def quantize_act(x, sx):
    """-> (codes int8 [rows, k], row sums int32 [rows])"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        t = (x / f32(sx)).astype(f32).astype(np.float64)
        r = np.sign(t) * np.floor(np.abs(t) + 0.5)                          # f32::round (exact in f64)
        r = np.clip(np.nan_to_num(r, nan=0.0, posinf=2147483647.0, neginf=-2147483648.0), -2147483648.0, 2147483647.0)
    q = np.clip(r.astype(np.int64), -128, 127).astype(np.int8)
    return q, q.astype(np.int64).sum(axis=-1).astype(np.int32)


def int_terms(qx, qw):
    """-> (t, rs) as int64: the caller may check them against int32.  (The product runs in float64, where it is exact: every partial
    sum is an integer below 2^14 K <= 2^30.)"""
    qx, qw = np.asarray(qx, np.int8), np.asarray(qw, np.int8)
    acc = (qx.astype(np.float64) @ qw.astype(np.float64).T).astype(np.int64)
    rs = qx.astype(np.int64).sum(axis=1)
    return acc + 128 * rs[:, None], rs


def linear_q8q8(qx, sx, qw, wparams, qb=None, bparams=None, relu=False):
    """qx [B, K] int8, qw [N, K] int8, wparams = (mw, sw) (th_quantize_int8's {min_val, scale}), qb [N] int8 with bparams = (mb, sb)"""
    assert np.asarray(qx).shape[1] == np.asarray(qw).shape[1] <= MAX_K
    t, rs = int_terms(qx, qw)
    assert np.abs(t).max(initial=0) < 2 ** 31
    mw, sw = f32(wparams[0]), f32(wparams[1])
    tf, rf = t.astype(np.int32).astype(f32), rs.astype(np.int32).astype(f32)[:, None]
    with np.errstate(all="ignore"):
        y = (f32(sx) * ((sw * tf).astype(f32) + (mw * rf).astype(f32)).astype(f32)).astype(f32)
        if qb is not None:
            y = (y + OX.dequantize_int8(qb, bparams[1], -128, bparams[0])[None, :]).astype(f32)
    return np.where(y > 0, y, f32(0)).astype(f32) if relu else y


def float64_linear(qx, sx, qw, wparams, qb=None, bparams=None):
    """the same product in float64 on the same decoded operands (the f32 values the codecs give, multiplied and summed in f64)"""
    xd = (np.asarray(qx, np.int8).astype(f32) * f32(sx)).astype(np.float64)
    wd = OX.dequantize_int8(np.asarray(qw, np.int8).reshape(-1), wparams[1], -128, wparams[0]).reshape(np.shape(qw)).astype(np.float64)
    y = xd @ wd.T
    return y + OX.dequantize_int8(qb, bparams[1], -128, bparams[0]).astype(np.float64)[None, :] if qb is not None else y


def float_layer(rng, B, K, N):
    """the issue's distributions: x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), b ~ 0.1 N(0, 1)"""
    x = rng.standard_normal((B, K)).astype(f32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(f32)
    b = (0.1 * rng.standard_normal(N)).astype(f32)
    return x, w, b


def pack(a):
    """-> (codes int8 of a's shape, (min_val, scale)) by the storage codec"""
    q, s, _, m = OX.quantize_int8(a)
    return q.reshape(np.shape(a)), (f32(m), f32(s))
