"""Numpy restatement of per-channel int8 weight scales (csrc/quant.hip's th_quantize_int8_channels and the _pc products) on top
of tests/qstatic_ref.py, tests/qconv_ref.py and tests/qchain_ref.py, exact to the bit:

    pack_channels   R.pack (the storage codec) of every channel alone: codes of the array's shape and one {min_val, scale} per channel
    linear_q8q8_pc  y[b][n] = sx * (sw[n] * (float)(acc + 128 rs) + mw[n] * (float)rs)  [+ dequantize_int8(qb[n])]  [max(y, 0)]
    conv_q8q8_pc    the same over im2col of the codes, n = the output channel

The integer terms are R.int_terms' and the four f32 operations keep R.linear_q8q8's order: with the same pair in every row both
restatements give the same bits."""
import numpy as np

from oracle import train_extra as OX
from tests import qconv_ref as Q
from tests import qstatic_ref as R

f32 = np.float32


def pack_channels(a, axis):
    """-> (codes int8 of a's shape, params f32 [channels, 2] = {min_val, scale}): the storage codec over each slice along `axis` alone"""
    a = np.asarray(a, f32)
    rows = np.moveaxis(a, axis, 0).reshape(a.shape[axis], -1)
    packed = [R.pack(r) for r in rows]
    codes = np.stack([q for q, _ in packed]).reshape(np.moveaxis(a, axis, 0).shape)
    return np.ascontiguousarray(np.moveaxis(codes, 0, axis)), np.array([p for _, p in packed], f32).reshape(-1, 2)


def same_pair(wparams, n):
    """one {mw, sw} repeated for n channels"""
    return np.tile(np.array(wparams, f32).reshape(1, 2), (n, 1))


def linear_q8q8_pc(qx, sx, qw, wparams, qb=None, bparams=None, relu=False):
    """qx [B, K] int8, qw [N, K] int8, wparams [N, 2] = {mw, sw} of every row of qw, qb [N] int8 with ONE pair bparams = (mb, sb)"""
    wparams = np.asarray(wparams, f32)
    assert np.asarray(qx).shape[1] == np.asarray(qw).shape[1] <= R.MAX_K and wparams.shape == (np.asarray(qw).shape[0], 2)
    t, rs = R.int_terms(qx, qw)
    assert np.abs(t).max(initial=0) < 2 ** 31
    mw, sw = wparams[None, :, 0], wparams[None, :, 1]
    tf, rf = t.astype(np.int32).astype(f32), rs.astype(np.int32).astype(f32)[:, None]
    with np.errstate(all="ignore"):
        y = (f32(sx) * ((sw * tf).astype(f32) + (mw * rf).astype(f32)).astype(f32)).astype(f32)
        if qb is not None:
            y = (y + OX.dequantize_int8(qb, bparams[1], -128, bparams[0])[None, :]).astype(f32)
    return np.where(y > 0, y, f32(0)).astype(f32) if relu else y


def float64_linear_pc(qx, sx, qw, wparams, qb=None, bparams=None):
    """the same product in float64 on the same decoded operands (every row of W decoded with its own pair)"""
    wparams = np.asarray(wparams, f32)
    xd = (np.asarray(qx, np.int8).astype(f32) * f32(sx)).astype(np.float64)
    wd = np.stack([OX.dequantize_int8(r, p[1], -128, p[0]) for r, p in zip(np.asarray(qw, np.int8), wparams)]).astype(np.float64)
    y = xd @ wd.T
    return y + OX.dequantize_int8(qb, bparams[1], -128, bparams[0]).astype(np.float64)[None, :] if qb is not None else y


def conv_q8q8_pc(qx, sx, qw, wparams, qb=None, bparams=None, stride=(1, 1), pad=(0, 0), relu=False):
    """qx [n, c_in, h, w] int8, qw [c_out, c_in, k_h, k_w] int8, wparams [c_out, 2] -> f32 [n, c_out, h_out, w_out]"""
    qx, qw = np.asarray(qx, np.int8), np.asarray(qw, np.int8)
    n, c, h, w = qx.shape
    co, ci, kh, kw = qw.shape
    assert ci == c and c * kh * kw <= R.MAX_K
    ho, wo = Q.out_hw(h, w, (kh, kw), stride, pad)
    y = linear_q8q8_pc(Q.im2col(qx, (kh, kw), stride, pad), sx, qw.reshape(co, -1), wparams, qb, bparams, relu)
    return np.ascontiguousarray(y.reshape(n, ho, wo, co).transpose(0, 3, 1, 2))


def conv_q8q8_codes_pc(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, sy, pitch):
    """tests/qchain_ref.py's conv_q8q8_codes on the per-channel product: -> (codes int8 [n, h_out, w_out, pitch] with zero padding bytes,
    pixel sums int32 [n, h_out, w_out]) through the same activation codec"""
    y = conv_q8q8_pc(qx, sx, qw, wparams, qb, bparams, stride, pad, relu)
    q, ps = Q.quantize_act_nchw(y, sy)
    return Q.nhwc(q, pitch), ps


def taper_pack_channels(flat, c_out, c_in, k):
    """a model's Conv2d buffer packed per EFFECTIVE output channel: the buffer read as [c_in k_h k_w][c_out] (Q.taper_weight), a pair per
    column -> (codes in the buffer's own order, flat; params [c_out, 2])"""
    q, p = pack_channels(np.asarray(flat, f32).reshape(c_in * k[0] * k[1], c_out), axis=1)
    return q.reshape(-1), p


def small_row_error(y, y64, n_mod=8, small_from=5):
    """the issue's metric: every output column's worst error against the float64 product relative to that column's own largest value, the
    worst over the small-magnitude columns n % 8 >= 5 (y [B, N]: column n is weight row n)"""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    err = np.abs(y - y64).max(axis=0) / np.abs(y64).max(axis=0)
    return float(err[np.arange(y.shape[1]) % n_mod >= small_from].max())


def scaled_rows_layer(seed, B=64, K=100, N=40):
    """the motivating construction: R.float_layer's distributions with weight row n multiplied by 2^-(n % 8)"""
    x, w, b = R.float_layer(np.random.default_rng(seed), B, K, N)
    return x, (w * (f32(2.0) ** -(np.arange(N) % 8).astype(f32))[:, None]).astype(f32), b
