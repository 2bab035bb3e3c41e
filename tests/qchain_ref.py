"""Numpy restatement of the int8 chain between static convolutions (csrc/qconv_i8.hip) on top of tests/qconv_ref.py, exact to the bit:

    conv_q8q8_codes = Q.conv_q8q8 (the f32 product, bias and ReLU included), then the activation codec with the NEXT layer's scale, then
                      channel-last: what th_quantize_act_nhwc_int8 makes of th_conv2d_q8q8_fwd's output
    max_pool_codes  = the maximum of the codes over the in-image taps, from -128 (the code of the float pool's -inf)

The codec clamp(round(v / s)) with s > 0 never decreases in v, so max_pool_codes(codec(x)) == codec(max_pool(x)) on finite x."""
import numpy as np

from tests import qconv_ref as Q

f32 = np.float32


def conv_q8q8_codes(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, sy, pitch):
    """-> (codes int8 [n, h_out, w_out, pitch] with zero padding bytes, pixel sums int32 [n, h_out, w_out])"""
    y = Q.conv_q8q8(qx, sx, qw, wparams, qb, bparams, stride, pad, relu)
    q, ps = Q.quantize_act_nchw(y, sy)
    return Q.nhwc(q, pitch), ps


def max_pool_codes(q, c, k, stride, pad=(0, 0)):
    """q int8 [n, h, w, pitch] (whatever its padding bytes hold) -> (codes [n, h_out, w_out, pitch] with zero padding bytes, pixel sums)"""
    q = np.asarray(q, np.int8)
    n, h, w, pitch = q.shape
    ho, wo = Q.out_hw(h, w, k, stride, pad)
    padded = np.full((n, h + 2 * pad[0], w + 2 * pad[1], pitch), -128, np.int8)
    padded[:, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = q
    out = np.full((n, ho, wo, pitch), -128, np.int8)
    for i in range(k[0]):
        for j in range(k[1]):
            out = np.maximum(out, padded[:, i:i + stride[0] * ho:stride[0], j:j + stride[1] * wo:stride[1]])
    out[..., c:] = 0
    return out, out[..., :c].astype(np.int64).sum(axis=-1).astype(np.int32)
