"""Quantization-aware training's boundary without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h), the Python face
(QATConfig, QATLinear, QATConv2d, the qat namespace) and the refusals, which happen before anything touches the device."""
import ctypes as C
import inspect

import pytest


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS
    for name, nargs in (("th_fake_quant_multi", 3), ("th_fake_quant_act", 6)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS
    for name, nargs in (("tp_qat_linear_new", 10), ("tp_qat_conv2d_new", 17), ("tp_qat_enable", 1), ("tp_qat_set_training", 1),
                        ("tp_qat_is_training", 1), ("tp_qat_module_set_enabled", 2), ("tp_qat_status", 4), ("tp_qat_module_observed", 2),
                        ("tp_qat_module_fake_quantized", 3)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name


def test_fq_item_struct_matches_the_header():
    from taper_amd import hip
    assert C.sizeof(hip.FqItem) == 40 and hip.FqItem.n.offset == 24 and hip.FqItem.qtype.offset == 32


def test_python_face():
    import taper_amd as T
    for cls in (T.QATLinear, T.QATConv2d):
        assert issubclass(cls, T.Module) and not issubclass(cls, (T.Linear, T.Conv2d))
        for meth in ("enable_qat", "observed", "fake_quantized", "quantize", "forward", "parameters"):
            assert callable(getattr(cls, meth))
    assert list(inspect.signature(T.QATConfig).parameters) == ["qtype", "activations", "symmetric", "per_channel"]
    c = T.QATConfig()
    assert (c.qtype, c.activations, c.symmetric, c.per_channel) == ("int8", True, True, False)
    for fn in ("enable", "disable", "set_training_mode", "is_training", "status"):
        assert callable(getattr(T.qat, fn))


def test_state_round_trips_without_a_device():
    import taper_amd as T
    assert T.qat.status()["global_enabled"] is False and T.qat.is_training()
    T.qat.enable()
    T.qat.set_training_mode(False)
    st = T.qat.status()
    assert st["global_enabled"] and not st["training_mode"] and not st["is_active"]
    T.qat.disable()
    T.qat.set_training_mode(True)
    assert T.qat.status()["global_enabled"] is False and T.qat.is_training()


@pytest.mark.parametrize("kw,match", [(dict(qtype="int4"), "placeholder"), (dict(qtype="bfloat16"), "placeholder"), (dict(qtype="nf4"), "placeholder"),
                                      (dict(symmetric=False), "symmetric"), (dict(per_channel=True), "per_channel"), (dict(qtype="int2"), "unknown")])
def test_refused_configs_raise_in_python(kw, match):
    import taper_amd as T
    with pytest.raises(T.TaperError, match=match):
        T.QATConfig(**kw)


@pytest.mark.parametrize("args,match", [((2, 1, 1, 0), "placeholder"), ((3, 1, 1, 0), "placeholder"), ((4, 1, 1, 0), "placeholder"),
                                        ((0, 1, 0, 0), "symmetric"), ((0, 1, 1, 1), "per_channel")])
def test_refused_configs_fail_in_the_host_before_the_device(args, match):
    # the C ABI refuses before any device work: no module is made, and on a machine without a GPU nothing else could have succeeded
    from taper_amd._lib import host
    out = C.c_void_p()
    assert host.tp_qat_linear_new(784, 10, 1, *args, None, 1, C.byref(out)) != 0 and out.value is None
    assert match in host.tp_last_error().decode()
    assert host.tp_qat_conv2d_new(1, 8, 3, 3, 1, 1, 1, 1, 1, 1, *args, b"c", 1, C.byref(out)) != 0 and out.value is None
    assert match in host.tp_last_error().decode()
