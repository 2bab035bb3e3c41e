"""A frozen BatchNorm2d in the quantized twins without a GPU: the C ABI declarations, the Python face, and the numpy
restatement itself (tests/qbn_ref.py) against the per-channel restatement and against float64."""
import inspect

import numpy as np

from tests import qbn_ref as N
from tests import qperchan_ref as P

f32 = np.float32


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    declared = parse_header(INCLUDE / "taper_hip.h")
    for name, nargs in (("th_fold_batchnorm2d", 8), ("th_channel_affine_fwd", 8), ("th_conv2d_q8q8_fwd_affine", 24), ("th_conv2d_q8q8_fwd_codes_affine", 27)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert name in declared and getattr(hip, name).argtypes == HIP_PROTOS[name][1], name
    # the twin's arguments, then int per_channel, then const float *d_affine
    for new, twin in (("th_conv2d_q8q8_fwd_affine", "th_conv2d_q8q8_fwd_pc"), ("th_conv2d_q8q8_fwd_codes_affine", "th_conv2d_q8q8_fwd_codes_pc")):
        assert HIP_PROTOS[new][0] == HIP_PROTOS[twin][0]
        assert HIP_PROTOS[new][1][:-2] == HIP_PROTOS[twin][1], new
        assert HIP_PROTOS[new][1][-2:] == [HIP_PROTOS["th_channel_affine_fwd"][1][3], HIP_PROTOS["th_channel_affine_fwd"][1][2]], new      # int, const float *
    # the older prototypes, unchanged
    for name, nargs in (("th_conv2d_q8q8_fwd", 22), ("th_conv2d_q8q8_fwd_pc", 22), ("th_conv2d_q8q8_fwd_codes", 25), ("th_conv2d_q8q8_fwd_codes_pc", 25),
                        ("th_batchnorm2d_fwd", 16), ("th_batchnorm2d_bwd", 15), ("th_debug_qconv_plan", 12), ("th_maxpool2d_nhwc_int8", 15)):
        assert len(HIP_PROTOS[name][1]) == nargs, name
    assert HIP_PROTOS["th_conv2d_q8q8_fwd_pc"] == HIP_PROTOS["th_conv2d_q8q8_fwd"] and HIP_PROTOS["th_conv2d_q8q8_fwd_codes_pc"] == HIP_PROTOS["th_conv2d_q8q8_fwd_codes"]


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, host
    for name, nargs in (("tp_qmodule_num_affines", 2), ("tp_qmodule_affine", 5)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name).argtypes == HOST_PROTOS[name][1]
    assert HOST_PROTOS["tp_qmodule_affine"] == HOST_PROTOS["tp_qmodule_tensor_params"]      # the same read-out shape
    for name, nargs in (("tp_module_quantize", 4), ("tp_module_quantize_static", 4), ("tp_module_quantize_static_conv", 4), ("tp_module_quantize_static_chain", 4),
                        ("tp_module_quantize_static_ex", 5), ("tp_qmodule_tensor", 5), ("tp_qmodule_storage_bytes", 2), ("tp_qmodule_act_scales", 4)):
        assert len(HOST_PROTOS[name][1]) == nargs, name      # unchanged


def test_python_face():
    import taper_amd as T
    assert list(inspect.signature(T.QuantizedModule.affines).parameters) == ["self"]
    for name in ("quantize_static", "quantize_static_conv", "quantize_static_chain"):      # unchanged
        assert list(inspect.signature(getattr(T.Module, name)).parameters) == ["self", "calib"], name
    assert list(inspect.signature(T.Module.quantize_static_per_channel).parameters) == ["self", "calib", "convs", "chain"]
    assert list(inspect.signature(T.Module.quantize).parameters) == ["self", "qtype", "enabled"]
    for name in ("tensors", "act_scales", "chain_links", "storage_bytes"):
        assert list(inspect.signature(getattr(T.QuantizedModule, name)).parameters) == ["self"], name


def _conv_case(rng):
    qx, qw = rng.integers(-128, 128, (2, 3, 6, 5)).astype(np.int8), rng.integers(-128, 128, (7, 3, 3, 3)).astype(np.int8)
    i = np.arange(7, dtype=f32)
    wp = np.stack([f32(-0.31) + f32(0.003) * i, f32(0.0024) * (f32(1) + f32(0.01) * i)], axis=1).astype(f32)
    return qx, qw, rng.integers(-128, 128, 7).astype(np.int8), wp


def test_the_identity_affine_gives_the_per_channel_restatements_values():
    qx, qw, qb, wp = _conv_case(np.random.default_rng(7))
    for bias, relu in ((0, 0), (1, 0), (1, 1)):
        ref = P.conv_q8q8_pc(qx, 0.0173, qw, wp, qb if bias else None, (-0.27, 0.0019), (1, 1), (1, 1), relu)
        got = N.conv_q8q8_affine(qx, 0.0173, qw, wp, qb if bias else None, (-0.27, 0.0019), (1, 1), (1, 1), relu, N.identity(7), True)
        assert got.dtype == np.float32 and np.array_equal(got, ref)      # as values: -0 + 0 is +0
        q1, s1 = N.conv_q8q8_codes_affine(qx, 0.0173, qw, wp, qb if bias else None, (-0.27, 0.0019), (1, 1), (1, 1), relu, N.identity(7), True, 0.05, 16)
        q2, s2 = P.conv_q8q8_codes_pc(qx, 0.0173, qw, wp, qb if bias else None, (-0.27, 0.0019), (1, 1), (1, 1), relu, 0.05, 16)
        np.testing.assert_array_equal(q1, q2)
        np.testing.assert_array_equal(s1, s2)
    one = N.conv_q8q8_affine(qx, 0.0173, qw, wp[3], None, None, (1, 1), (0, 0), False, N.identity(7), False)      # one pair: the per-tensor product
    np.testing.assert_array_equal(one, P.conv_q8q8_pc(qx, 0.0173, qw, P.same_pair(wp[3], 7), None, None, (1, 1), (0, 0), False))


def test_the_affine_comes_before_the_relu_and_rounds_twice():
    qx, qw, qb, wp = _conv_case(np.random.default_rng(8))
    ab = np.stack([np.array([-1.5, 0.0, 0.75, 1.0, -0.25, 2.0, 1e-3], f32), np.array([0.1, 0.2, -0.3, 0.0, 0.5, -4.0, 0.0], f32)], axis=1)
    v = P.conv_q8q8_pc(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), False)
    got = N.conv_q8q8_affine(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), True, ab, True)
    for ch in range(7):
        want = np.maximum(f32(v[:, ch] * ab[ch, 0]) + ab[ch, 1], f32(0))
        np.testing.assert_array_equal(got[:, ch], want.astype(f32))
    assert (got[:, 0][v[:, 0] > 1] == 0).all() and (got[:, 1] == f32(0.2)).all()      # a negative a flips the sign; a zero a leaves b


def test_fold_agrees_with_float64():
    rng = np.random.default_rng(11)
    c = 4096
    var = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), c)).astype(f32)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32)
    beta, mean = (0.1 * rng.standard_normal(c)).astype(f32), rng.standard_normal(c).astype(f32)
    for eps in (1e-5, 1e-3):
        ab = N.fold(gamma, beta, mean, var, eps)
        assert ab.dtype == np.float32 and ab.shape == (c, 2)
        a64 = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(f32(eps)))
        b64 = beta.astype(np.float64) - mean.astype(np.float64) * a64
        err_a = float((np.abs(ab[:, 0] - a64) / np.abs(a64)).max())
        # b is a difference: its error is relative to the terms it is made of
        err_b = float((np.abs(ab[:, 1] - b64) / (np.abs(beta) + np.abs(mean.astype(np.float64) * a64))).max())
        print(f"fold vs float64, eps {eps}: a {err_a:.3e}, b {err_b:.3e}")
        assert err_a <= 1e-6 and err_b <= 1e-6
    zero = N.fold([2.0, 0.0, -1.0], [0.5, 0.25, 0.0], [1.0, 3.0, -2.0], [0.0, 1.0, 0.0], 1e-5)      # var == 0, gamma == 0
    inv = f32(1) / np.sqrt(f32(1e-5))
    np.testing.assert_array_equal(zero[:, 0], np.array([f32(2) * inv, 0, -inv], f32))
    assert zero[1, 1] == f32(0.25)
