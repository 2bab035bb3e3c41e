"""Per-channel int8 weight scales without a GPU: the C ABI declarations, the Python face, and the numpy restatement itself
(tests/qperchan_ref.py) against the per-tensor restatements, against float64, and on the construction that motivates it."""
import inspect

import numpy as np
import pytest

from tests import qconv_ref as Q
from tests import qperchan_ref as P
from tests import qstatic_ref as R

f32 = np.float32


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    for name, nargs in (("th_quantize_int8_channels", 8), ("th_linear_q8q8_fwd_pc", 15), ("th_conv2d_q8q8_fwd_pc", 22), ("th_conv2d_q8q8_fwd_codes_pc", 25)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert name in parse_header(INCLUDE / "taper_hip.h") and getattr(hip, name).argtypes == HIP_PROTOS[name][1]
    for pc, twin in (("th_linear_q8q8_fwd_pc", "th_linear_q8q8_fwd"), ("th_conv2d_q8q8_fwd_pc", "th_conv2d_q8q8_fwd"),
                     ("th_conv2d_q8q8_fwd_codes_pc", "th_conv2d_q8q8_fwd_codes")):
        assert HIP_PROTOS[pc] == HIP_PROTOS[twin], pc      # the same arguments: only the meaning of d_wparams changes


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, INCLUDE, host
    for name, nargs in (("tp_module_quantize_static_ex", 5), ("tp_qmodule_tensor_channels", 5), ("tp_qmodule_tensor_params", 5)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name).argtypes == HOST_PROTOS[name][1]
    for name, nargs in (("tp_module_quantize_static", 4), ("tp_module_quantize_static_conv", 4), ("tp_module_quantize_static_chain", 4), ("tp_qmodule_tensor", 5)):
        assert len(HOST_PROTOS[name][1]) == nargs, name      # unchanged
    text = (INCLUDE / "taper_host.h").read_text()
    for flag, value in (("TP_QSTATIC_CONVS", 1), ("TP_QSTATIC_CHAIN", 2), ("TP_QSTATIC_PER_CHANNEL", 4)):
        assert f"#define {flag} {value}\n" in text, flag


def test_python_face():
    import taper_amd as T
    assert list(inspect.signature(T.Module.quantize_static_per_channel).parameters) == ["self", "calib", "convs", "chain"]
    sig = inspect.signature(T.Module.quantize_static_per_channel).parameters
    assert sig["convs"].default is True and sig["chain"].default is True
    assert list(inspect.signature(T.QuantizedModule.channel_layout).parameters) == ["self", "i"]
    for name in ("quantize_static", "quantize_static_conv", "quantize_static_chain"):      # unchanged
        assert list(inspect.signature(getattr(T.Module, name)).parameters) == ["self", "calib"], name
    assert list(inspect.signature(T.Module.quantize).parameters) == ["self", "qtype", "enabled"]
    assert list(inspect.signature(T.QuantizedModule.tensors).parameters) == ["self"]
    assert list(inspect.signature(T.QuantizedModule.act_scales).parameters) == ["self"]


def test_pack_channels_is_the_storage_codec_of_every_channel():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 7)).astype(f32)
    a[2] = 0.25                                            # a constant channel: the +-0.1 widening
    for axis in (0, 1):
        q, p = P.pack_channels(a, axis)
        assert q.shape == a.shape and q.dtype == np.int8 and p.shape == (a.shape[axis], 2) and p.dtype == f32
        for c in range(a.shape[axis]):
            qc, pc = R.pack(np.take(a, c, axis))
            np.testing.assert_array_equal(np.take(q, c, axis), qc)
            np.testing.assert_array_equal(p[c], np.array(pc, f32))
    np.testing.assert_array_equal(P.pack_channels(a, 0)[1][2], np.array([f32(0.25) - f32(0.1), f32(f32(0.25) + f32(0.1) - (f32(0.25) - f32(0.1))) / f32(255)]))
    flat = rng.standard_normal(3 * 9 * 4).astype(f32)      # a Conv2d buffer [c_out 4, c_in 3, 3, 3]: a pair per column of [27][4]
    q, p = P.taper_pack_channels(flat, 4, 3, (3, 3))
    for co in range(4):
        qc, pc = R.pack(Q.taper_weight(flat, 4, 3, (3, 3))[co])
        np.testing.assert_array_equal(Q.taper_weight(q, 4, 3, (3, 3))[co], qc)
        np.testing.assert_array_equal(p[co], np.array(pc, f32))


@pytest.mark.parametrize("wp", [(0.0, 1.0), (-0.31, 0.0024)])
def test_the_same_pair_in_every_row_is_the_per_tensor_restatement_bit_for_bit(wp):
    rng = np.random.default_rng(7)
    qx, qw, qb = rng.integers(-128, 128, (9, 70)).astype(np.int8), rng.integers(-128, 128, (33, 70)).astype(np.int8), rng.integers(-128, 128, 33).astype(np.int8)
    for sx, bias, relu in ((1.0, 0, 0), (0.0173, 1, 0), (0.0173, 1, 1)):
        a = P.linear_q8q8_pc(qx, sx, qw, P.same_pair(wp, 33), qb if bias else None, (-0.27, 0.0019), relu)
        b = R.linear_q8q8(qx, sx, qw, wp, qb if bias else None, (-0.27, 0.0019), relu)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    cx, cw = rng.integers(-128, 128, (2, 3, 6, 5)).astype(np.int8), rng.integers(-128, 128, (7, 3, 3, 3)).astype(np.int8)
    a = P.conv_q8q8_pc(cx, 0.0173, cw, P.same_pair(wp, 7), qb[:7], (-0.27, 0.0019), (1, 1), (1, 1), True)
    b = Q.conv_q8q8(cx, 0.0173, cw, wp, qb[:7], (-0.27, 0.0019), (1, 1), (1, 1), True)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("B,K,N", [(5, 784, 128), (33, 100, 10), (130, 4096, 70)])
def test_reference_is_within_1e6_of_float64_on_the_same_operands(B, K, N):
    """tests/test_qstatic_abi.py's bound and shapes: four f32 roundings per output against the float64 product of the decoded operands"""
    rng = np.random.default_rng(0)
    for b, k, n in ((5, 784, 128), (33, 100, 10), (130, 4096, 70)):      # one stream, the shapes in the issue's order
        x, w, bias = R.float_layer(rng, b, k, n)
        if (b, k, n) == (B, K, N):
            break
    sx = R.act_scale_of(x)
    qx, _ = R.quantize_act(x, sx)
    qw, wp = P.pack_channels(w, 0)
    qb, bp = R.pack(bias)
    y, y64 = P.linear_q8q8_pc(qx, sx, qw, wp, qb, bp), P.float64_linear_pc(qx, sx, qw, wp, qb, bp)
    err = float(np.abs(y - y64).max() / np.abs(y64).max())
    print(f"per-channel reference vs float64 at {(B, K, N)}: {err:.3e} of max |y|")
    assert y.dtype == np.float32 and err <= 1e-6, err
    assert len({tuple(p) for p in wp}) == N                # every row has a pair of its own


@pytest.mark.parametrize("seed", range(5))
def test_per_row_scales_recover_the_small_rows(seed):
    """The motivating construction: Linear 100 -> 40, R.float_layer's distributions at batch 64, weight row n multiplied by 2^-(n % 8).
    A per-tensor step is 1 / 255 of the LARGEST row's range, the size of a whole small row (n % 8 >= 5: at most 1 / 32 of it), so those
    output columns are noise; a per-row step is 1 / 255 of the row's own range.  Measured on the CPU: per-tensor 0.96 to 1.67 of the
    column's largest value, per-row 1.35e-2 to 1.64e-2, a factor of 58 to 106; the condition is a factor of 10."""
    x, w, _ = P.scaled_rows_layer(seed)
    sx = R.act_scale_of(x)
    qx, _ = R.quantize_act(x, sx)
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    per_tensor = P.small_row_error(R.linear_q8q8(qx, sx, *R.pack(w)), y64)
    per_row = P.small_row_error(P.linear_q8q8_pc(qx, sx, *P.pack_channels(w, 0)), y64)
    print(f"seed {seed}: per-tensor {per_tensor:.3e}, per-row {per_row:.3e}, factor {per_tensor / per_row:.1f}")
    assert per_row <= per_tensor / 10, (per_tensor, per_row)
