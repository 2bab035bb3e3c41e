"""Numpy restatement of the calibrated int8 convolution (csrc/qconv_i8.hip) on top of tests/qstatic_ref.py, exact to the bit:

    qx  = the activation codec of the Linear restatement, per element of x [n, c, h, w]; pixsum[n, h, w] = sum over channels
    col = im2col of the CODES ([n h_out w_out, c_in k_h k_w]; an out-of-image tap is code 0, which IS value 0)
    y   = R.linear_q8q8(col, sx, qw.reshape(c_out, -1), ...)  -> [n, c_out, h_out, w_out]

A row sum of col is the sum of the pixel sums over the window's in-image taps, so linear_q8q8's rs is the kernel's rs."""
import numpy as np

from tests import qstatic_ref as R

f32 = np.float32
MAX_K = R.MAX_K


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad[0] - k[0]) // stride[0] + 1, (w + 2 * pad[1] - k[1]) // stride[1] + 1


def cpitch(c):
    return -(-c // 16) * 16


def quantize_act_nchw(x, sx):
    """x [n, c, h, w] -> (codes int8 [n, c, h, w], pixel sums int32 [n, h, w])"""
    x = np.asarray(x, f32)
    q, _ = R.quantize_act(x.reshape(-1, 1), sx)
    q = q.reshape(x.shape)
    return q, q.astype(np.int64).sum(axis=1).astype(np.int32)


def nhwc(q, pitch, fill=0):
    """codes [n, c, h, w] -> [n, h, w, pitch] with the padding bytes set to `fill`"""
    n, c, h, w = q.shape
    out = np.full((n, h, w, pitch), fill, np.int8)
    out[..., :c] = q.transpose(0, 2, 3, 1)
    return out


def pack_weight(qw, pitch, fill=0):
    """codes [c_out, c_in, k_h, k_w] -> [c_out, k_h * k_w, pitch]"""
    co, ci, kh, kw = qw.shape
    out = np.full((co, kh * kw, pitch), fill, np.int8)
    out[..., :ci] = qw.reshape(co, ci, kh * kw).transpose(0, 2, 1)
    return out


def taper_weight(flat, c_out, c_in, k):
    """the filters a model's Conv2d applies: its [c_out, c_in, k_h, k_w] buffer read as [c_in k_h k_w][c_out] (the float conv kernels'
    weight_layout 0, tensor.rs:1262) -> standard [c_out, c_in, k_h, k_w]"""
    return np.ascontiguousarray(np.asarray(flat).reshape(c_in * k[0] * k[1], c_out).T).reshape(c_out, c_in, k[0], k[1])


def im2col(q, k, stride, pad):
    """q [n, c, h, w] (any dtype) -> [n * h_out * w_out, c * k_h * k_w], zero outside the image; columns in (c, k_h, k_w) order"""
    n, c, h, w = q.shape
    ho, wo = out_hw(h, w, k, stride, pad)
    padded = np.zeros((n, c, h + 2 * pad[0], w + 2 * pad[1]), q.dtype)
    padded[:, :, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = q
    col = np.empty((n, ho, wo, c, k[0], k[1]), q.dtype)
    for i in range(k[0]):
        for j in range(k[1]):
            col[:, :, :, :, i, j] = padded[:, :, i:i + stride[0] * ho:stride[0], j:j + stride[1] * wo:stride[1]].transpose(0, 2, 3, 1)
    return col.reshape(n * ho * wo, c * k[0] * k[1])


def conv_q8q8(qx, sx, qw, wparams, qb=None, bparams=None, stride=(1, 1), pad=(0, 0), relu=False):
    """qx [n, c_in, h, w] int8, qw [c_out, c_in, k_h, k_w] int8 -> f32 [n, c_out, h_out, w_out]"""
    qx, qw = np.asarray(qx, np.int8), np.asarray(qw, np.int8)
    n, c, h, w = qx.shape
    co, ci, kh, kw = qw.shape
    assert ci == c and c * kh * kw <= MAX_K
    ho, wo = out_hw(h, w, (kh, kw), stride, pad)
    y = R.linear_q8q8(im2col(qx, (kh, kw), stride, pad), sx, qw.reshape(co, -1), wparams, qb, bparams, relu)
    return np.ascontiguousarray(y.reshape(n, ho, wo, co).transpose(0, 3, 1, 2))


def float64_conv(qx, sx, qw, wparams, qb=None, bparams=None, stride=(1, 1), pad=(0, 0)):
    """the same convolution in float64 on the decoded operands"""
    qx, qw = np.asarray(qx, np.int8), np.asarray(qw, np.int8)
    n, c, h, w = qx.shape
    co, _, kh, kw = qw.shape
    ho, wo = out_hw(h, w, (kh, kw), stride, pad)
    y = R.float64_linear(im2col(qx, (kh, kw), stride, pad), sx, qw.reshape(co, -1), wparams, qb, bparams)
    return y.reshape(n, ho, wo, co).transpose(0, 3, 1, 2)


def max_pool(x, k, stride):
    """exact: a maximum of f32 values (no padding)"""
    n, c, h, w = x.shape
    ho, wo = (h - k[0]) // stride[0] + 1, (w - k[1]) // stride[1] + 1
    out = np.full((n, c, ho, wo), -np.inf, f32)
    for i in range(k[0]):
        for j in range(k[1]):
            out = np.maximum(out, x[:, :, i:i + stride[0] * ho:stride[0], j:j + stride[1] * wo:stride[1]])
    return out


def float_layer(rng, n, c_in, h, w, c_out, k):
    """the issue's distributions: x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), b ~ 0.1 N(0, 1)"""
    K = c_in * k[0] * k[1]
    x = rng.standard_normal((n, c_in, h, w)).astype(f32)
    wt = (rng.standard_normal((c_out, c_in, k[0], k[1])) / np.sqrt(K)).astype(f32)
    b = (0.1 * rng.standard_normal(c_out)).astype(f32)
    return x, wt, b
