"""Numpy restatement of a frozen BatchNorm2d in the quantized twins (csrc/quant.hip's th_fold_batchnorm2d and th_channel_affine_fwd, the
AFFINE form of csrc/qconv_i8.hip) on top of tests/qconv_ref.py, tests/qperchan_ref.py and tests/qchain_ref.py, exact to the bit:

    fold                    invstd = 1 / sqrt(var + eps), a = gamma * invstd, b = beta - mean * a  -> [c, 2] = {a, b}
    affine                  y[:, ch] * a[ch] + b[ch], then max(., 0) with relu
    conv_q8q8_affine        the product's value, bias included and WITHOUT its ReLU (one weight pair, or one per output channel), then affine
    conv_q8q8_codes_affine  that through the activation codec with the next layer's scale, channel-last

Every array is float32, so each operation rounds once, in the order written."""
import numpy as np

from tests import qchain_ref as CH  # noqa: F401  (max_pool_codes: what a link's pool does to these codes)
from tests import qconv_ref as Q
from tests import qperchan_ref as P

f32 = np.float32


def fold(gamma, beta, mean, var, eps):
    gamma, beta, mean, var = (np.asarray(v, f32) for v in (gamma, beta, mean, var))
    with np.errstate(all="ignore"):
        invstd = (f32(1) / np.sqrt((var + f32(eps)).astype(f32)).astype(f32)).astype(f32)
        a = (gamma * invstd).astype(f32)
        b = (beta - (mean * a).astype(f32)).astype(f32)
    return np.stack([a, b], axis=1)


def affine(y, ab, relu=False):
    """y f32 [n, c, h, w], ab [c, 2]"""
    y, ab = np.asarray(y, f32), np.asarray(ab, f32)
    assert y.ndim == 4 and ab.shape == (y.shape[1], 2)
    with np.errstate(all="ignore"):
        out = ((y * ab[None, :, 0, None, None]).astype(f32) + ab[None, :, 1, None, None]).astype(f32)
    return np.where(out > 0, out, f32(0)).astype(f32) if relu else out


def conv_q8q8_affine(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel):
    """wparams: [c_out, 2] with per_channel, one pair without -> f32 [n, c_out, h_out, w_out]"""
    v = (P.conv_q8q8_pc if per_channel else Q.conv_q8q8)(qx, sx, qw, wparams, qb, bparams, stride, pad, False)
    return affine(v, ab, relu)


def conv_q8q8_codes_affine(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel, sy, pitch):
    """-> (codes int8 [n, h_out, w_out, pitch] with zero padding bytes, pixel sums int32 [n, h_out, w_out])"""
    q, ps = Q.quantize_act_nchw(conv_q8q8_affine(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel), sy)
    return Q.nhwc(q, pitch), ps


def identity(c):
    """a = 1, b = 0: the affine that changes no value (-0 aside: -0 + 0 = +0)"""
    return np.stack([np.ones(c, f32), np.zeros(c, f32)], axis=1)
