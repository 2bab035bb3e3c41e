"""Quantized residual models without a GPU: the C ABI declarations, the TP_QBLOCKS flag, the Python face, and the numpy
restatement itself (tests/qres_ref.py) against tests/qbn_ref.py and against float64."""
import inspect

import numpy as np

from tests import qbn_ref as N
from tests import qconv_ref as Q
from tests import qres_ref as S

f32 = np.float32
F32_FN, CODES_FN = "th_conv2d_q8q8_fwd_residual", "th_conv2d_q8q8_fwd_codes_residual"


def test_kernel_entry_points_are_declared_and_exported():
    import ctypes as C

    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    declared = parse_header(INCLUDE / "taper_hip.h")
    for name, nargs in ((F32_FN, 28), (CODES_FN, 31)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert name in declared and getattr(hip, name).argtypes == HIP_PROTOS[name][1], name
    # the affine twin's arguments, then const float *d_res, const int8_t *d_res_q, int cpitch_r, const float *d_res_scale
    for new, twin in ((F32_FN, "th_conv2d_q8q8_fwd_affine"), (CODES_FN, "th_conv2d_q8q8_fwd_codes_affine")):
        assert HIP_PROTOS[new][0] == HIP_PROTOS[twin][0]
        assert HIP_PROTOS[new][1][:-4] == HIP_PROTOS[twin][1], new
        assert HIP_PROTOS[new][1][-4:] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], new
    for name, nargs in (("th_conv2d_q8q8_fwd_affine", 24), ("th_conv2d_q8q8_fwd_codes_affine", 27), ("th_conv2d_q8q8_fwd", 22), ("th_conv2d_q8q8_fwd_codes", 25),
                        ("th_debug_qconv_plan", 12)):
        assert len(HIP_PROTOS[name][1]) == nargs, name      # unchanged


def test_a_call_without_a_context_is_refused_by_name():
    from taper_amd._lib import hip
    shared = (None, 16, None, None, 1, 3, 4, 4, None, 8, 3, 3, 1, 1, 1, 1, None, None, None, 1)
    assert hip.th_conv2d_q8q8_fwd_residual(None, *shared, None, 0, None, None, None, 0, None) != 0
    assert F32_FN.encode() in hip.th_last_error()
    assert hip.th_conv2d_q8q8_fwd_codes_residual(None, *shared, None, None, 16, None, 0, None, None, None, 0, None) != 0
    assert CODES_FN.encode() in hip.th_last_error()


def test_the_flag_and_the_host_entry_points():
    from taper_amd._lib import HOST_PROTOS, INCLUDE
    text = (INCLUDE / "taper_host.h").read_text()
    assert "#define TP_QBLOCKS 32" in text
    assert text.count("#define TP_QSTATIC_") == 4      # the new flag is not one of them: bit 8 stays unknown
    for name, nargs in (("tp_module_quantize_static_ex", 5), ("tp_module_quantize_static_cal", 8), ("tp_module_quantize", 4), ("tp_qmodule_chain_links", 2)):
        assert len(HOST_PROTOS[name][1]) == nargs, name      # unchanged


def test_python_face():
    import taper_amd as T
    sig = inspect.signature(T.Module.quantize_static_residual)
    assert list(sig.parameters) == ["self", "calib", "chain", "per_channel", "links", "percentile", "bins"]
    assert [p.default for p in sig.parameters.values()][2:] == [True, False, False, None, 2048]
    for name in ("quantize_static", "quantize_static_conv", "quantize_static_chain"):      # unchanged
        assert list(inspect.signature(getattr(T.Module, name)).parameters) == ["self", "calib"], name
    assert list(inspect.signature(T.Module.quantize_static_per_channel).parameters) == ["self", "calib", "convs", "chain"]
    assert list(inspect.signature(T.Module.quantize_static_linked).parameters) == ["self", "calib", "per_channel"]
    assert list(inspect.signature(T.Module.quantize_static_calibrated).parameters) == ["self", "calib", "percentile", "bins", "convs", "chain", "per_channel", "links"]


def _conv_case(rng, c_out=7):
    qx, qw = rng.integers(-128, 128, (2, 3, 6, 5)).astype(np.int8), rng.integers(-128, 128, (c_out, 3, 3, 3)).astype(np.int8)
    i = np.arange(c_out, dtype=f32)
    wp = np.stack([f32(-0.31) + f32(0.003) * i, f32(0.0024) * (f32(1) + f32(0.01) * i)], axis=1).astype(f32)
    ab = np.stack([(f32(0.5) + f32(0.1) * i) * np.where(np.arange(c_out) % 2, f32(-1), f32(1)), f32(0.37) * (i - 3)], axis=1).astype(f32)
    return qx, qw, rng.integers(-128, 128, c_out).astype(np.int8), wp, ab


def test_the_codes_form_is_the_codec_of_the_f32_form():
    rng = np.random.default_rng(3)
    qx, qw, qb, wp, ab = _conv_case(rng)
    res = rng.standard_normal((2, 7, 6, 5)).astype(f32)
    res_q = rng.integers(-128, 128, (2, 7, 6, 5)).astype(np.int8)
    for kw in (dict(res=res), dict(res_q=res_q, res_scale=0.02)):
        for relu in (False, True):
            y = S.conv_q8q8_residual(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), relu, ab, True, **kw)
            assert y.dtype == np.float32 and y.shape == (2, 7, 6, 5) and (y.min() >= 0) == relu
            q, ps = S.conv_q8q8_codes_residual(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), relu, ab, True, 0.05, 16, **kw)
            ref_q, ref_ps = Q.quantize_act_nchw(y, 0.05)
            np.testing.assert_array_equal(q, Q.nhwc(ref_q, 16))
            np.testing.assert_array_equal(ps, ref_ps)
            assert not q[..., 7:].any()


def test_integer_codes_with_scale_one_are_the_f32_residual_of_the_same_values():
    rng = np.random.default_rng(4)
    qx, qw, qb, wp, ab = _conv_case(rng)
    res_q = rng.integers(-128, 128, (2, 7, 6, 5)).astype(np.int8)
    for pc, w in ((True, wp), (False, wp[2])):
        a = S.conv_q8q8_residual(qx, 0.0173, qw, w, qb, (-0.27, 0.0019), (1, 1), (1, 1), True, ab, pc, res_q=res_q, res_scale=1.0)
        b = S.conv_q8q8_residual(qx, 0.0173, qw, w, qb, (-0.27, 0.0019), (1, 1), (1, 1), True, ab, pc, res=res_q.astype(f32))
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_zero_residual_reproduces_the_affine_restatement():
    rng = np.random.default_rng(5)
    qx, qw, qb, wp, ab = _conv_case(rng)
    for relu in (False, True):
        ref = N.conv_q8q8_affine(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), relu, ab, True)
        a = S.conv_q8q8_residual(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), relu, ab, True, res=np.zeros((2, 7, 6, 5), f32))
        b = S.conv_q8q8_residual(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), relu, ab, True, res_q=np.zeros((2, 7, 6, 5), np.int8), res_scale=0.3)
        assert np.array_equal(a, ref) and np.array_equal(b, ref)      # as values: -0 + 0 is +0


def test_the_residual_comes_behind_the_affine_and_before_the_relu():
    rng = np.random.default_rng(6)
    qx, qw, qb, wp, ab = _conv_case(rng)
    res = (5 * rng.standard_normal((2, 7, 6, 5))).astype(f32)
    res.reshape(-1)[:3] = np.nan, np.inf, -np.inf
    v = N.conv_q8q8_affine(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), False, ab, True)
    got = S.conv_q8q8_residual(qx, 0.0173, qw, wp, qb, (-0.27, 0.0019), (1, 1), (1, 1), True, ab, True, res=res)
    with np.errstate(all="ignore"):
        want = (v + res).astype(f32)
    want = np.where(want > 0, want, f32(0))
    np.testing.assert_array_equal(got, want)
    assert got.reshape(-1)[0] == 0 and np.isposinf(got.reshape(-1)[1]) and got.reshape(-1)[2] == 0      # max(NaN, 0) = 0


def _seeded_block(kind):
    """seed 0 of the construction the closeness bound was measured on: w ~ N(0, 1) / sqrt(K), gamma in +-[0.5, 1.5], beta ~ 0.1 N(0, 1),
    running mean ~ 0.3 N(0, 1), running var in [0.5, 2], x ~ N(0, 1) on [4, 8, 8, 8]"""
    rng = np.random.default_rng(0)

    def bn(c):
        return S.bn_spec(rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c), 0.1 * rng.standard_normal(c), 0.3 * rng.standard_normal(c), rng.uniform(0.5, 2.0, c))

    def w(co, ci, k):
        return (rng.standard_normal(co * ci * k * k) / np.sqrt(ci * k * k)).astype(f32)

    if kind == "residual":
        blk = S.residual_block([w(8, 8, 3), w(8, 8, 3)], [bn(8), bn(8)], 8, 8, 1)
    else:
        blk = S.bottleneck_block([w(4, 8, 1), w(4, 4, 3), w(16, 4, 1), w(16, 8, 1)], [bn(4), bn(4), bn(16), bn(16)], 8, 4, 16, 2)
    return blk, rng.standard_normal((4, 8, 8, 8)).astype(f32)


def test_the_restated_block_twins_stay_close_to_float64():
    """The restatement alone: an identity ResidualBlock(8, 8, 1) and a BottleneckBlock(8, 4, 16, 2) on [4, 8, 8, 8], calibrated on the
    test's own input, against the float block in float64, max |error| over max |y|.  Measured on the CPU for this seed: residual 1.406e-2
    per-tensor and 1.113e-2 per-channel, bottleneck 9.967e-3 and 1.066e-2; seeds 0 .. 7 give 0.88e-2 .. 1.47e-2 (residual) and 0.73e-2 ..
    1.16e-2 (bottleneck).  The bound is twice this seed's figure: seeds vary by about that much, a wrong layout, fold or residual is off
    by the order of max |y| itself."""
    measured = {("residual", False): 1.406e-2, ("residual", True): 1.113e-2, ("bottleneck", False): 9.967e-3, ("bottleneck", True): 1.066e-2}
    for (kind, pc), m in measured.items():
        blk, x = _seeded_block(kind)
        scales = S.block_calibration_scales(blk, x)
        y = S.block_twin(blk, x, scales, pc)
        ref = S.block_float64(blk, x)
        assert y.dtype == np.float32 and y.shape == ref.shape == ((4, 8, 8, 8) if kind == "residual" else (4, 16, 4, 4))
        err = float(np.abs(y - ref).max() / np.abs(ref).max())
        print(f"restated {kind} twin, per_channel {pc}, vs float64: {err:.3e} of max |y| (measured {m:.3e})")
        assert err <= 2 * m, (kind, pc, err)
    blk, x = _seeded_block("bottleneck")
    assert len(S.block_calibration_scales(blk, x)) == 4 and S.block_calibration_scales(blk, x)[0] == S.block_calibration_scales(blk, x)[3]
