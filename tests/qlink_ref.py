"""Numpy restatement of the int8 links through the classifier (csrc/qgemm_i8.hip's th_linear_q8q8_fwd_link) on top of
tests/qstatic_ref.py, tests/qperchan_ref.py and tests/qconv_ref.py, exact to the bit:

    linear_q8q8_codes = the f32 product (R.linear_q8q8 or P.linear_q8q8_pc: bias and ReLU included), then the activation codec with the
                        NEXT layer's scale, rows padded with the code 0 to its pitch: what th_quantize_act_int8 makes of the product
    row_sums          = the int32 sum of every row's codes, padding included (the code 0 adds nothing)
    relay_flatten     = a Linear's rows [c][HW] (the columns Flatten gives an NCHW map) as [HW][cpitch], zero in the padded channels:
                        the weight a channel-last map of codes [HW][cpitch] meets element by element

Every sum is over integers, so the order of the columns cannot reach the bits."""
import numpy as np

from tests import qperchan_ref as P
from tests import qstatic_ref as R

f32 = np.float32


def up16(n):
    return -(-n // 16) * 16


def linear_f32(qx, sx, qw, wparams, qb=None, bparams=None, relu=False):
    """the f32 product: wparams of shape [N, 2] is a pair per row (P.linear_q8q8_pc), a single pair R.linear_q8q8"""
    pc = np.ndim(wparams) == 2
    return (P.linear_q8q8_pc if pc else R.linear_q8q8)(qx, sx, qw, wparams, qb, bparams, relu)


def linear_q8q8_codes(qx, sx, qw, wparams, qb, bparams, relu, sy, pitch):
    """-> codes int8 [B, pitch]: column n < N the code of the product's value, the rest 0"""
    q, _ = R.quantize_act(linear_f32(qx, sx, qw, wparams, qb, bparams, relu), sy)
    assert pitch % 16 == 0 and pitch >= q.shape[1]
    out = np.zeros((q.shape[0], pitch), np.int8)
    out[:, :q.shape[1]] = q
    return out


def row_sums(q):
    """q int8 [rows, pitch] -> int32 [rows]"""
    return np.asarray(q, np.int8).astype(np.int64).sum(axis=1).astype(np.int32)


def relay_flatten(qw, c, hw, cpitch, fill=0):
    """qw int8 [out, c * hw] (column ch * hw + p) -> [out, hw * cpitch] (column p * cpitch + ch), the padded channels `fill`"""
    qw = np.asarray(qw, np.int8)
    out = np.full((qw.shape[0], hw, cpitch), fill, np.int8)
    out[:, :, :c] = qw.reshape(-1, c, hw).transpose(0, 2, 1)
    return out.reshape(qw.shape[0], hw * cpitch)


def flatten_nhwc(q_nchw, cpitch):
    """codes [n, c, h, w] -> the rows a Flatten link reads: [n, h * w * cpitch], zero in the padded channels"""
    n, c, h, w = q_nchw.shape
    out = np.zeros((n, h, w, cpitch), np.int8)
    out[..., :c] = q_nchw.transpose(0, 2, 3, 1)
    return out.reshape(n, h * w * cpitch)
