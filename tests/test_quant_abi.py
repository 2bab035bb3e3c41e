"""Post-training quantization's boundary without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h) and the
Python face (Module.quantize -> QuantizedModule)."""
import inspect

import pytest


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS
    for name, nargs in (("th_linear_q8_fwd", 11), ("th_linear_h16_fwd", 9), ("th_dequantize_multi", 3), ("th_qlinear_stream_max_batch", 0)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS
    for name, nargs in (("tp_module_quantize", 4), ("tp_qmodule_forward", 3), ("tp_qmodule_storage_bytes", 2), ("tp_qmodule_num_tensors", 2),
                        ("tp_qmodule_tensor_len", 3), ("tp_qmodule_tensor", 5), ("tp_qmodule_free", 1)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name


def test_qtensor_struct_matches_the_header():
    import ctypes as C

    from taper_amd import hip
    assert C.sizeof(hip.QTensor) == 40 and hip.QTensor.n.offset == 24 and hip.QTensor.qtype.offset == 32


def test_python_face():
    import taper_amd as T
    assert callable(T.Module.quantize) and T.QuantizedModule.__call__ is T.QuantizedModule.forward
    assert list(inspect.signature(T.Module.quantize).parameters) == ["self", "qtype", "enabled"]
    assert set(T.QuantizedModule.QTYPES) == {"int8", "float16", "int4", "bfloat16", "nf4"}
    for meth in ("forward", "storage_bytes", "tensors"):
        assert callable(getattr(T.QuantizedModule, meth))


def test_unknown_qtype_is_refused_before_the_device():
    import taper_amd as T
    m = T.Module.__new__(T.Module)
    m._h = None
    with pytest.raises(T.TaperError, match="unknown qtype"):
        m.quantize("int2")
