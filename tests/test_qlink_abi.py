"""Int8 links through the classifier without a GPU: the C ABI declarations, the flag, the Python face, and the numpy
restatement itself (tests/qlink_ref.py): the codes of a product are the codec of its f32 restatement, and a product on re-laid
channel-last codes is the product on the flattened NCHW codes."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import qconv_ref as Q
from tests import qlink_ref as L
from tests import qperchan_ref as P
from tests import qstatic_ref as R

f32 = np.float32
FN = "th_linear_q8q8_fwd_link"


def test_kernel_entry_point_is_declared_exported_and_prototyped():
    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    assert FN in HIP_PROTOS and FN in parse_header(INCLUDE / "taper_hip.h")
    ret, args = HIP_PROTOS[FN]
    assert ret is C.c_int and getattr(hip, FN).argtypes == args
    p, i = C.c_void_p, C.c_int
    #               ctx qx pitch_x rowsum xscale batch K  qw pitch_w N  wparams pc qb bparams relu y  yscale qy pitch_y
    assert args == [p, p, i, p, p, i, i, p, i, i, p, i, p, p, i, p, p, p, i]
    # th_linear_q8q8_fwd's list with per_channel put in behind d_wparams and the destination behind it: nothing else moved
    old = HIP_PROTOS["th_linear_q8q8_fwd"][1]
    assert args[:11] == old[:11] and args[12:16] == old[11:] and HIP_PROTOS["th_linear_q8q8_fwd_pc"][1] == old


def test_flag_and_host_entry_points():
    from taper_amd._lib import HOST_PROTOS, INCLUDE
    text = (INCLUDE / "taper_host.h").read_text()
    for flag, value in (("TP_QSTATIC_CONVS", 1), ("TP_QSTATIC_CHAIN", 2), ("TP_QSTATIC_PER_CHANNEL", 4), ("TP_QSTATIC_LINKS", 16)):
        assert f"#define {flag} {value}\n" in text, flag
    assert "#define TP_QSTATIC_" in text and text.count("#define TP_QSTATIC_") == 4      # bit 8 stays unknown
    assert len(HOST_PROTOS["tp_module_quantize_static_ex"][1]) == 5 and len(HOST_PROTOS["tp_qmodule_chain_links"][1]) == 2


def test_python_face():
    import taper_amd as T
    from taper_amd import api
    sig = inspect.signature(T.Module.quantize_static_linked).parameters
    assert list(sig) == ["self", "calib", "per_channel"] and sig["per_channel"].default is False
    assert api._QSTATIC_LINKS == 16
    for name in ("quantize_static", "quantize_static_conv", "quantize_static_chain"):      # unchanged
        assert list(inspect.signature(getattr(T.Module, name)).parameters) == ["self", "calib"], name
    assert list(inspect.signature(T.Module.quantize_static_per_channel).parameters) == ["self", "calib", "convs", "chain"]
    assert "Linear" in T.QuantizedModule.chain_links.__doc__ and "Flatten" in T.QuantizedModule.chain_links.__doc__


def test_a_call_without_a_context_is_refused_by_name():
    from taper_amd._lib import hip
    assert getattr(hip, FN)(None, None, 16, None, None, 1, 1, None, 16, 1, None, 0, None, None, 0, None, None, None, 0) != 0
    assert hip.th_last_error().decode() == FN + ": null argument"


def test_the_plan_describes_the_link_call_too():
    from taper_amd._lib import hip
    out = (C.c_int * 4)()
    for B, N, want in ((1, 1, (1, 1, 1, 1)), (256, 33, (1, 8, 2, 16)), (257, 129, (0, 3, 2, 6))):
        assert hip.th_debug_q8q8_plan(B, 64, N, C.cast(out, C.c_void_p)) == 0 and tuple(out) == want


# ---------------------------------------------------------------- the restatement's own identities
@pytest.mark.parametrize("pc", [0, 1])
@pytest.mark.parametrize("bias,relu", [(0, 0), (1, 0), (1, 1)])
def test_codes_are_the_codec_of_the_f32_restatement(pc, bias, relu):
    rng = np.random.default_rng(10 * pc + 2 * bias + relu)
    B, K, N = 9, 37, 21
    x, w, b = R.float_layer(rng, B, K, N)
    sx = R.act_scale_of(x)
    qx, _ = R.quantize_act(x, sx)
    (qw, wp), (qb, bp) = (P.pack_channels(w, 0) if pc else R.pack(w)), R.pack(b)
    y = (P.linear_q8q8_pc if pc else R.linear_q8q8)(qx, sx, qw, wp, qb if bias else None, bp, relu)
    sy = f32(R.act_scale_of(y) * f32(0.6))
    for pitch in (32, 96):
        q = L.linear_q8q8_codes(qx, sx, qw, wp, qb if bias else None, bp, relu, sy, pitch)
        ref, rs = R.quantize_act(y, sy)
        assert q.shape == (B, pitch) and q.dtype == np.int8 and (q[:, N:] == 0).all()
        np.testing.assert_array_equal(q[:, :N], ref)
        np.testing.assert_array_equal(L.row_sums(q), rs)      # the padding adds nothing to a row's sum
        assert np.abs(q.astype(int)).max() >= 127 and len(np.unique(q)) > 8      # the codes spread and saturate
    with pytest.raises(AssertionError):
        L.linear_q8q8_codes(qx, sx, qw, wp, None, None, relu, sy, 16)      # a pitch below N


@pytest.mark.parametrize("c,h,w,n_out", [(6, 2, 2, 12), (1, 3, 5, 4), (17, 1, 1, 3), (16, 2, 3, 5)])
def test_product_on_relaid_channel_last_codes_is_the_product_on_flattened_codes(c, h, w, n_out):
    rng = np.random.default_rng(c * 100 + h * 10 + w)
    q_nchw = rng.integers(-128, 128, (3, c, h, w)).astype(np.int8)
    qw = rng.integers(-128, 128, (n_out, c * h * w)).astype(np.int8)
    cp = Q.cpitch(c)
    flat = q_nchw.reshape(3, -1)                                   # what Flatten(1) gives: column ch * hw + p
    rows, relaid = L.flatten_nhwc(q_nchw, cp), L.relay_flatten(qw, c, h * w, cp)
    assert rows.shape == (3, h * w * cp) and relaid.shape == (n_out, h * w * cp)
    t0, rs0 = R.int_terms(flat, qw)
    t1, rs1 = R.int_terms(rows, relaid)
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(rs0, rs1)
    np.testing.assert_array_equal(rs1.astype(np.int32), L.row_sums(rows))
    for sx, wp in ((1.0, (0.0, 1.0)), (0.0173, (-0.31, 0.0024))):
        np.testing.assert_array_equal(R.linear_q8q8(flat, sx, qw, wp).view(np.uint32), R.linear_q8q8(rows, sx, relaid, wp).view(np.uint32))
    # whatever the weight's padded channels hold, they meet the code 0
    np.testing.assert_array_equal(R.int_terms(rows, L.relay_flatten(qw, c, h * w, cp, fill=0x55))[0], t0)
