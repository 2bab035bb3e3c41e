"""The exact pointwise convolution and BottleneckBlock without a GPU: the libraries export every new entry point with the declared signature,
the flag constant has its value, the Python face has the stated signatures and leaves the pinned ones alone, and what is refused on the host
is refused before anything touches the device."""
import ctypes as C
import inspect
import re

import pytest

I, P, U64 = C.c_int, C.c_void_p, C.c_uint64
# name -> argument types behind ctx
TH = {
    "th_conv1x1_exact_fwd": [P, P, P, P] + [I] * 8,            # x, w, bias, y; n, c_in, h, w, c_out, stride, weight_layout, relu
    "th_conv1x1_exact_bwd_input": [P, P, P] + [I] * 8,         # gy, w, gx; n, c_in, h, w, c_out, stride, weight_layout, accumulate
    "th_conv1x1_exact_bwd_weight": [P, P, P] + [I] * 8,        # x, gy, gw; ...
}
TH_DEBUG = {
    "th_debug_conv1x1_exact_plan": [I] * 11 + [P],             # op, n, c_in, h, w, c_out, stride, layout, relu_bias, accumulate, misalign; out
    "th_debug_last_conv_pw_config": [P, P],                    # ctx, out
}
TP = {
    "tp_bottleneck_block_new": [I, I, I, I, U64, P],           # in, mid, out, stride, seed; out
    "tp_conv2d_ex": [P, P, P] + [I] * 8 + [P],
    "tp_conv2d_new_ex": [I] * 10 + [U64, I, P],
    "tp_residual_block_new_ex": [I, I, I, U64, I, P],
    "tp_basic_block_new_ex": [I, I, I, U64, I, P],
}


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, INCLUDE, hip, parse_header
    public, debug = parse_header(INCLUDE / "taper_hip.h"), parse_header(INCLUDE / "taper_hip_debug.h")
    for name, args in TH.items():
        assert name in public and name not in debug, name
        assert HIP_PROTOS[name] == (I, [P] + args), (name, HIP_PROTOS[name])
        assert getattr(hip, name)
    for name, args in TH_DEBUG.items():
        assert name in debug and name not in public, name
        assert HIP_PROTOS[name] == (I, args), (name, HIP_PROTOS[name])
        assert getattr(hip, name)
    # the default 1x1 entry point and the stride-2 3x3 family keep their signatures
    assert len(HIP_PROTOS["th_conv1x1_fwd"][1]) == 12
    assert [len(HIP_PROTOS[f"th_conv3x3_s2_{k}"][1]) for k in ("fwd", "bwd_input", "bwd_weight")] == [12, 11, 11]
    assert len(HIP_PROTOS["th_debug_conv3x3_s2_plan"][1]) == 11 and len(HIP_PROTOS["th_debug_conv3x3_plan"][1]) == 13


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, INCLUDE, host
    for name, args in TP.items():
        assert HOST_PROTOS[name] == (I, args), (name, HOST_PROTOS[name])
        assert getattr(host, name)
    text = (INCLUDE / "taper_host.h").read_text()
    assert re.search(r"^#define TP_CONV_EXACT_POINTWISE 16$", text, re.M) and re.search(r"^#define TP_CONV_EXACT_STRIDE 1$", text, re.M)
    import taper_amd.api as api
    assert api.EXACT_POINTWISE == 16 and api.EXACT_STRIDE == 1


def _tail(fn, n):
    sig = inspect.signature(fn)
    return [(k, v.default) for k, v in list(sig.parameters.items())[-n:]]


def test_python_face():
    import taper_amd as T
    assert "BottleneckBlock" in T.__all__ and issubclass(T.BottleneckBlock, T.Module)
    # exact_pointwise=False is appended after exact_stride
    for fn in (T.Tensor.conv2d, T.Tensor.conv2d_relu, T.Conv2d.__init__, T.Conv2dReLU.__init__):
        assert _tail(fn, 2) == [("exact_stride", False), ("exact_pointwise", False)], fn
    assert list(inspect.signature(T.Tensor.conv2d).parameters)[1:] == ["weight", "bias", "stride", "padding", "dilation", "relu", "exact_stride",
                                                                      "exact_pointwise"]
    sig = inspect.signature(T.ResidualBlock.pointwise_shortcut)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty),
                                                                    ("stride", 1), ("seed", 1), ("exact_stride", True)]
    assert isinstance(inspect.getattr_static(T.ResidualBlock, "pointwise_shortcut"), classmethod)
    sig = inspect.signature(T.BottleneckBlock.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("in_channels", inspect.Parameter.empty), ("mid_channels", inspect.Parameter.empty),
                                                                              ("out_channels", inspect.Parameter.empty), ("stride", 1), ("seed", 1)]
    # the pinned constructors are unchanged
    for cls in (T.ResidualBlock, T.BasicBlock):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters)[1:] == ["in_channels", "out_channels", "stride", "seed"], cls
        assert sig.parameters["stride"].default == 1 and sig.parameters["seed"].default == 1


def test_bad_arguments_are_refused_before_the_device_is_touched():
    # on a machine without a GPU nothing that needs the device could have succeeded: the refusal and its message come from the host
    import taper_amd as T
    from taper_amd._lib import host
    out = C.c_void_p()
    for args in ((0, 4, 8, 1), (8, 0, 8, 1), (8, 4, 0, 1), (8, 4, 8, 0), (-1, 4, 8, 1)):
        assert host.tp_bottleneck_block_new(*args, 1, C.byref(out)) != 0 and out.value is None, args
        assert "must be positive" in host.tp_last_error().decode()
    assert host.tp_bottleneck_block_new(8, 4, 8, 3, 1, C.byref(out)) != 0 and out.value is None
    assert "BottleneckBlock: the stride must be 1 or 2 (got 3)" in host.tp_last_error().decode()
    assert host.tp_bottleneck_block_new(8, 4, 8, 1, 1, None) != 0 and "null argument" in host.tp_last_error().decode()
    with pytest.raises(T.TaperError, match="BottleneckBlock: the stride must be 1 or 2 \\(got 4\\)"):
        T.BottleneckBlock(8, 4, 8, 4)
    with pytest.raises(T.TaperError, match="Conv2d exact_pointwise: the kernel must be 1x1 \\(got 3x3\\)"):
        T.Conv2d(4, 8, (3, 3), exact_pointwise=True)
    with pytest.raises(T.TaperError, match="Conv2d exact_pointwise: the stride must be \\(1, 1\\) or \\(2, 2\\) \\(got \\(3, 3\\)\\)"):
        T.Conv2d(4, 8, (1, 1), (3, 3), exact_pointwise=True)
    with pytest.raises(T.TaperError, match="Conv2d exact_pointwise: groups must be 1 \\(got 2\\)"):
        T.Conv2d(4, 8, (1, 1), groups=2, exact_pointwise=True)
    with pytest.raises(T.TaperError, match="ResidualBlock pointwise_shortcut: the stride must be 1 or 2 \\(got 3\\)"):
        T.ResidualBlock.pointwise_shortcut(4, 8, 3, exact_stride=False)
    # the flag word: only the bits that are unknown are printed
    for fn, args in (("tp_conv2d_new_ex", (4, 8, 1, 1, 1, 1, 0, 0, 1, 0, 1)), ("tp_residual_block_new_ex", (4, 8, 2, 1))):
        for flags, unknown in ((2, 2), (4, 4), (8, 8), (18, 2), (31, 14)):
            assert getattr(host, fn)(*args, flags, C.byref(out)) != 0 and out.value is None
            assert f"{fn}: unknown flag bits {unknown} " in host.tp_last_error().decode(), (fn, flags, host.tp_last_error())
    assert host.tp_basic_block_new_ex(4, 8, 2, 1, 16, C.byref(out)) != 0 and out.value is None
    assert "tp_basic_block_new_ex: unknown flag bits 16 " in host.tp_last_error().decode()
    # the kernel entry points refuse by name before any launch
    from taper_amd._lib import hip
    for name in TH:
        assert getattr(hip, name)(None, *([None] * (len(TH[name]) - 8)), 1, 1, 1, 1, 1, 1, 0, 0) != 0
        assert f"{name}: null argument".encode() in hip.th_last_error()
