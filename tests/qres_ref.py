"""Numpy restatement of a skip connection in the int8 conv epilogue (the RES forms of csrc/qconv_i8.hip) on top of
tests/qbn_ref.py, exact to the bit:

    residual_value            ((v * a[ch]) + b[ch]) + r, then max(., 0) with relu (NaN -> 0 there)
    conv_q8q8_residual        the product's value, bias included and WITHOUT its ReLU, then residual_value with r = res (an f32 map of
                              the output's shape) or r = res_q * res_scale (int8 codes [n, c_out, h_out, w_out] and their scale)
    conv_q8q8_codes_residual  that through the activation codec with the next layer's scale, channel-last

Every array is float32, so each operation rounds once, in the order written."""
import numpy as np

from tests import qbn_ref as N
from tests import qconv_ref as Q
from tests import qperchan_ref as P
from tests import qstatic_ref as R

f32 = np.float32


def residual_of_codes(res_q, res_scale):
    """codes int8 [n, c, h, w] and their scale -> the f32 values the epilogue adds: one multiply"""
    with np.errstate(all="ignore"):
        return (np.asarray(res_q, np.int8).astype(f32) * f32(res_scale)).astype(f32)


def residual_value(v, ab, r, relu=False):
    """v, r f32 [n, c, h, w], ab [c, 2]"""
    v, ab, r = np.asarray(v, f32), np.asarray(ab, f32), np.asarray(r, f32)
    assert v.ndim == 4 and ab.shape == (v.shape[1], 2) and r.shape == v.shape
    with np.errstate(all="ignore"):
        y = (N.affine(v, ab, False) + r).astype(f32)
    return np.where(y > 0, y, f32(0)).astype(f32) if relu else y


def conv_q8q8_residual(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel, res=None, res_q=None, res_scale=None):
    """exactly one of res (f32) and res_q (int8 codes, with res_scale), both [n, c_out, h_out, w_out] -> f32 of that shape"""
    assert (res is None) != (res_q is None) and (res_q is None or res_scale is not None)
    v = (P.conv_q8q8_pc if per_channel else Q.conv_q8q8)(qx, sx, qw, wparams, qb, bparams, stride, pad, False)
    r = np.asarray(res, f32) if res is not None else residual_of_codes(res_q, res_scale)
    return residual_value(v, ab, r, relu)


def conv_q8q8_codes_residual(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel, sy, pitch, res=None, res_q=None, res_scale=None):
    """-> (codes int8 [n, h_out, w_out, pitch] with zero padding bytes, pixel sums int32 [n, h_out, w_out])"""
    y = conv_q8q8_residual(qx, sx, qw, wparams, qb, bparams, stride, pad, relu, ab, per_channel, res, res_q, res_scale)
    q, ps = Q.quantize_act_nchw(y, sy)
    return Q.nhwc(q, pitch), ps


# ---------------------------------------------------------------- the block twins (QuantizeOptions::blocks)
def conv_spec(w, c_out, c_in, k, stride, pad):
    """a block's conv: its float buffer (flat, read as [c_in k_h k_w][c_out] like every conv the twins take) and its geometry"""
    w = np.asarray(w, f32).reshape(-1)
    assert w.size == c_out * c_in * k[0] * k[1]
    return dict(w=w, c_out=c_out, c_in=c_in, k=k, stride=stride, pad=pad)


def bn_spec(gamma, beta, mean, var, eps=1e-5):
    return dict(gamma=np.asarray(gamma, f32), beta=np.asarray(beta, f32), mean=np.asarray(mean, f32), var=np.asarray(var, f32), eps=eps)


def residual_block(weights, bns, in_ch, out_ch, stride, pointwise=False):
    """ResidualBlock(in, out, stride) from its conv buffers (conv1, conv2, [projection]) and bn_spec's (bn1, bn2, [the shortcut's]); every
    conv is a convolution: 3x3 / pad 1 at `stride`, the projection 3x3 / pad 1 or, with `pointwise`, 1x1 / pad 0 at `stride`"""
    s = (stride, stride)
    main = [(conv_spec(weights[0], out_ch, in_ch, (3, 3), s, (1, 1)), bns[0]), (conv_spec(weights[1], out_ch, out_ch, (3, 3), (1, 1), (1, 1)), bns[1])]
    proj = None
    if in_ch != out_ch or stride != 1:
        proj = (conv_spec(weights[2], out_ch, in_ch, (1, 1) if pointwise else (3, 3), s, (0, 0) if pointwise else (1, 1)), bns[2])
    assert len(weights) == len(bns) == 2 + (proj is not None)
    return dict(main=main, proj=proj)


def bottleneck_block(weights, bns, in_ch, mid_ch, out_ch, stride):
    """BottleneckBlock(in, mid, out, stride): 1x1 -> 3x3 / pad 1 at `stride` -> 1x1, the projection 1x1 at `stride`"""
    s = (stride, stride)
    main = [(conv_spec(weights[0], mid_ch, in_ch, (1, 1), (1, 1), (0, 0)), bns[0]), (conv_spec(weights[1], mid_ch, mid_ch, (3, 3), s, (1, 1)), bns[1]),
            (conv_spec(weights[2], out_ch, mid_ch, (1, 1), (1, 1), (0, 0)), bns[2])]
    proj = (conv_spec(weights[3], out_ch, in_ch, (1, 1), s, (0, 0)), bns[3]) if in_ch != out_ch or stride != 1 else None
    assert len(weights) == len(bns) == 3 + (proj is not None)
    return dict(main=main, proj=proj)


def block_convs(block):
    """(conv, bn) in the twin's order: conv1, conv2, [conv3], [projection]"""
    return block["main"] + ([block["proj"]] if block["proj"] else [])


def pack_conv(cv, per_channel):
    """-> (codes [c_out, c_in, k_h, k_w] as the product reads them, one weight pair or [c_out, 2])"""
    if per_channel:
        q, p = P.taper_pack_channels(cv["w"], cv["c_out"], cv["c_in"], cv["k"])
    else:
        q, p = R.pack(cv["w"])
    return Q.taper_weight(np.asarray(q).reshape(-1), cv["c_out"], cv["c_in"], cv["k"]), p


def block_twin(block, x, scales, per_channel):
    """The block's twin on an f32 input [n, c, h, w]; scales: conv1, conv2, [conv3], [projection] (the projection's equals conv1's).
    A boundary crossed in int8 gives the same codes as the codec on the f32 value, so one restatement stands for every form."""
    parts = block_convs(block)
    assert len(scales) == len(parts)
    packs = [pack_conv(cv, per_channel) for cv, _ in parts]
    abs_ = [N.fold(bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["eps"]) for _, bn in parts]
    qin, _ = Q.quantize_act_nchw(x, scales[0])
    q, nmain = qin, len(block["main"])
    for i in range(nmain - 1):
        cv = parts[i][0]
        y = N.conv_q8q8_affine(q, scales[i], packs[i][0], packs[i][1], None, None, cv["stride"], cv["pad"], True, abs_[i], per_channel)
        q, _ = Q.quantize_act_nchw(y, scales[i + 1])
    i, cv = nmain - 1, parts[nmain - 1][0]
    if block["proj"]:
        pv = parts[-1][0]
        kw = dict(res=N.conv_q8q8_affine(qin, scales[-1], packs[-1][0], packs[-1][1], None, None, pv["stride"], pv["pad"], False, abs_[-1], per_channel))
    else:
        kw = dict(res_q=qin, res_scale=scales[0])
    return conv_q8q8_residual(q, scales[i], packs[i][0], packs[i][1], None, None, cv["stride"], cv["pad"], True, abs_[i], per_channel, **kw)


def float64_conv(x, cv):
    """a real convolution in float64 with the filters the float kernels apply"""
    w = Q.taper_weight(cv["w"], cv["c_out"], cv["c_in"], cv["k"]).astype(np.float64)
    n, c, h, wd = x.shape
    ho, wo = Q.out_hw(h, wd, cv["k"], cv["stride"], cv["pad"])
    col = Q.im2col(np.asarray(x, np.float64), cv["k"], cv["stride"], cv["pad"])
    return (col @ w.reshape(cv["c_out"], -1).T).reshape(n, ho, wo, cv["c_out"]).transpose(0, 3, 1, 2)


def float64_bn(x, bn):
    g, b, m, v = (bn[k].astype(np.float64)[None, :, None, None] for k in ("gamma", "beta", "mean", "var"))
    return (x - m) / np.sqrt(v + np.float64(f32(bn["eps"]))) * g + b


def block_float64(block, x):
    """the float block in eval mode, in float64"""
    x = np.asarray(x, np.float64)
    shortcut = float64_bn(float64_conv(x, block["proj"][0]), block["proj"][1]) if block["proj"] else x
    h = x
    for cv, bn in block["main"][:-1]:
        h = np.maximum(float64_bn(float64_conv(h, cv), bn), 0)
    cv, bn = block["main"][-1]
    return np.maximum(float64_bn(float64_conv(h, cv), bn) + shortcut, 0)


def block_calibration_scales(block, x):
    """the min / max scales a calibration on the one tensor x gives the block's convs, from the float block in f32-rounded float64"""
    x = np.asarray(x, np.float64)
    h, scales = x, []
    for cv, bn in block["main"]:
        scales.append(R.act_scale_of(h.astype(f32)))
        h = np.maximum(float64_bn(float64_conv(h, cv), bn), 0)
    if block["proj"]:
        scales.append(scales[0])
    return scales
