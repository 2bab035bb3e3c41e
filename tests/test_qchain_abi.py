"""The int8 chain between static convolutions without a GPU: the C ABI declarations and the Python face, the width limit of the
product that writes codes, the coverage of the GPU test's case table through the plan the launch consumes, and the identity the chained
twin rests on -- a max-pool commutes with the activation codec -- on the numpy restatements (tests/qchain_ref.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import qchain_ref as QC
from tests import qconv_ref as Q
from tests import qstatic_ref as R

f32 = np.float32


def test_entry_points_are_declared_exported_and_prototyped():
    from taper_amd._lib import HIP_PROTOS, HOST_PROTOS, INCLUDE, hip, host, parse_header
    for name, nargs in (("th_qconv_i8_chain_max_cout", 0), ("th_conv2d_q8q8_fwd_codes", 25), ("th_maxpool2d_nhwc_int8", 15)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name
        assert name in parse_header(INCLUDE / "taper_hip.h") and getattr(hip, name).argtypes == HIP_PROTOS[name][1]
    # the arguments of th_conv2d_q8q8_fwd up to and including relu, then the scale, the codes, their pitch and the pixel sums
    assert HIP_PROTOS["th_conv2d_q8q8_fwd_codes"][1][:21] == HIP_PROTOS["th_conv2d_q8q8_fwd"][1][:21]
    assert HIP_PROTOS["th_conv2d_q8q8_fwd_codes"][1][21:] == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    for name, nargs in (("tp_module_quantize_static_chain", 4), ("tp_qmodule_chain_links", 2)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name).argtypes == HOST_PROTOS[name][1]
    assert HOST_PROTOS["tp_module_quantize_static_chain"] == HOST_PROTOS["tp_module_quantize_static_conv"]


def test_python_face():
    import taper_amd as T
    assert list(inspect.signature(T.Module.quantize_static_chain).parameters) == ["self", "calib"]
    assert list(inspect.signature(T.QuantizedModule.chain_links).parameters) == ["self"]
    assert list(inspect.signature(T.Module.quantize_static_conv).parameters) == ["self", "calib"]      # unchanged


def test_one_workgroup_covers_128_channels():
    from taper_amd._lib import hip
    from tests.test_gpu_qconv import plan
    assert hip.th_qconv_i8_chain_max_cout() == 128
    assert plan(1, 16, 8, 8, 128, (3, 3), (1, 1), (1, 1))["tiles_n"] == 1 and plan(1, 16, 8, 8, 129, (3, 3), (1, 1), (1, 1))["tiles_n"] == 2


def test_case_table_reaches_every_form_and_edge():
    from tests.test_gpu_qchain import assert_case_table_coverage
    assert_case_table_coverage()


POOLS = [((2, 2), (2, 2)), ((3, 3), (2, 2)), ((3, 2), (1, 2))]


@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "k{}x{}-s{}{}".format(*p[0], *p[1]))
def test_max_pool_commutes_with_the_codec(pool):
    """20 random tensors with zeros mixed in, under scales from "nothing saturates" to "most of the data saturates": pooling the codes
    gives the codes of the pooled floats, element for element"""
    k, s = pool
    rng = np.random.default_rng(100 + k[0] * 10 + k[1])
    saturated = 0
    for t in range(20):
        n, c, h, w = int(rng.integers(1, 4)), int(rng.integers(1, 20)), int(rng.integers(3, 12)), int(rng.integers(3, 12))
        x = (rng.standard_normal((n, c, h, w)) * rng.choice([0.01, 1.0, 300.0])).astype(f32)
        x[rng.random(x.shape) < 0.3] = 0                                     # what a ReLU leaves
        scale = f32(R.act_scale_of(x) * rng.choice([1.0, 0.5, 0.05]))        # below 1: part of the data lies outside the range
        q, _ = Q.quantize_act_nchw(x, scale)
        saturated += int((np.abs(q.astype(int)) >= 127).sum() > 1)
        pitch = Q.cpitch(c) + 16 * (t % 2)
        got, sums = QC.max_pool_codes(Q.nhwc(q, pitch, fill=0x55), c, k, s)
        ref_q, ref_sums = Q.quantize_act_nchw(Q.max_pool(x, k, s), scale)
        np.testing.assert_array_equal(got, Q.nhwc(ref_q, pitch))
        np.testing.assert_array_equal(sums, ref_sums)
    assert saturated >= 5


def test_an_empty_window_is_the_code_of_minus_infinity():
    """padding as large as the window: the corner windows hold no tap.  The float pool leaves -inf there and the codec maps it to -128,
    the integer pool's start value"""
    q = np.random.default_rng(1).integers(-128, 128, (1, 4, 4, 16)).astype(np.int8)
    got, sums = QC.max_pool_codes(q, 3, (2, 2), (2, 2), pad=(2, 2))
    assert got.shape == (1, 4, 4, 16) and (got[0, 0, 0, :3] == -128).all() and sums[0, 0, 0] == -384
    assert Q.quantize_act_nchw(np.array([[[[-np.inf]]]], f32), 0.1)[0].item() == -128
    np.testing.assert_array_equal(got[0, 1:3, 1:3], QC.max_pool_codes(q, 3, (2, 2), (2, 2))[0][0])      # the inner windows are the unpadded pool's


def test_padding_bytes_of_both_restatements_are_zero():
    rng = np.random.default_rng(2)
    qx = rng.integers(-128, 128, (2, 3, 6, 5)).astype(np.int8)
    qw = rng.integers(-128, 128, (5, 3, 3, 3)).astype(np.int8)
    for pitch in (16, 48):
        codes, sums = QC.conv_q8q8_codes(qx, 0.02, qw, (-0.3, 0.0024), None, None, (1, 1), (1, 1), True, 0.4, pitch)
        assert codes.shape == (2, 6, 5, pitch) and codes.dtype == np.int8 and not codes[..., 5:].any() and codes[..., :5].any()
        np.testing.assert_array_equal(sums, codes.astype(np.int64).sum(axis=-1))
        pooled, psums = QC.max_pool_codes(np.where(np.arange(pitch) < 5, codes, 0x55).astype(np.int8), 5, (2, 2), (2, 2))
        assert pooled.shape == (2, 3, 2, pitch) and not pooled[..., 5:].any()
        np.testing.assert_array_equal(psums, pooled.astype(np.int64).sum(axis=-1))
    # the codes are the codec of the f32 product, channel-last
    y = Q.conv_q8q8(qx, 0.02, qw, (-0.3, 0.0024), None, None, (1, 1), (1, 1), True)
    np.testing.assert_array_equal(codes[..., :5], Q.quantize_act_nchw(y, 0.4)[0].transpose(0, 2, 3, 1))
