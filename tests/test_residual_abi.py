"""The residual tail and ResidualBlock without a GPU: the float64 restatement the GPU tests compare against (tests/residual_ref.py) agrees
with the torch fixtures of tests/golden/make_golden_residual.py; the libraries export the four new entry points; the Python face exists
with its signatures; and what is refused on the host is refused before anything touches the device."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest

from tests import residual_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden"
TH = (("th_bn_residual_fwd", 16), ("th_bn_residual_bwd", 15))      # (arguments behind ctx)
TP = (("tp_batchnorm2d_forward_add", 4), ("tp_residual_block_new", 5))
BOUND = 1e-9   # of the tensor's scale: both sides are float64


def _close(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-300)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= BOUND, (name, err)


@pytest.mark.parametrize("name", ["residual_tail_2x5x3x3", "residual_tail_4x3x1x1"])
def test_reference_agrees_with_the_torch_fixture(name):
    g = np.load(GOLDEN / f"{name}.npz")
    for mode, training in (("t", True), ("e", False)):
        for tag, relu in (("p", False), ("r", True)):
            k = f"{mode}{tag}"
            f = R.forward(g["x"], g["r"], g["gamma"], g["beta"], g["rm0"], g["rv0"], 1e-5, 0.1, training, relu)
            _close(f"y_{k}", f["y"], g[f"y_{k}"])
            _close(f"rm_{k}", f["running_mean"], g[f"rm_{k}"])
            _close(f"rv_{k}", f["running_var"], g[f"rv_{k}"])
            if not training:
                assert np.array_equal(f["running_mean"], g["rm0"]) and np.array_equal(f["running_var"], g["rv0"])
            gx, gr, gg, gb = R.backward(g["gy"], g["x"], g["gamma"], f["save_mean"], f["save_invstd"], f["y"] if relu else None, training)
            _close(f"gx_{k}", gx, g[f"gx_{k}"])
            _close(f"gr_{k}", gr, g[f"gr_{k}"])
            _close(f"gg_{k}", gg, g[f"gg_{k}"])
            _close(f"gb_{k}", gb, g[f"gb_{k}"])
            if relu:
                assert (g[f"gr_{k}"] == 0).any() and (g[f"gr_{k}"] != 0).any(), "the fixture's ReLU masks some elements and keeps others"


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, hip
    for name, nargs in TH:
        assert name in HIP_PROTOS, name
        assert len(HIP_PROTOS[name][1]) == nargs + 1, name
        assert getattr(hip, name)
    fwd = HIP_PROTOS["th_bn_residual_fwd"][1]
    assert fwd[10] is C.c_int and fwd[13] is C.c_float and fwd[14] is C.c_float     # n; eps, momentum
    # the plain family keeps its three entries: the fused tail is not one of them
    assert {n for n in HIP_PROTOS if n.startswith("th_batchnorm")} == {"th_batchnorm2d_fwd", "th_batchnorm2d_bwd", "th_batchnorm2d_split"}
    assert len(HIP_PROTOS["th_batchnorm2d_fwd"][1]) == 16 and len(HIP_PROTOS["th_batchnorm2d_bwd"][1]) == 15


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, host
    for name, nargs in TP:
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name)


def test_python_face():
    import taper_amd as T
    assert "ResidualBlock" in T.__all__ and "BatchNorm2d" in T.__all__
    sig = inspect.signature(T.ResidualBlock.__init__)
    assert list(sig.parameters)[1:] == ["in_channels", "out_channels", "stride", "seed"]
    assert sig.parameters["stride"].default == 1 and sig.parameters["seed"].default == 1
    sig = inspect.signature(T.BatchNorm2d.forward_add)
    assert list(sig.parameters)[1:] == ["x", "residual"]
    assert list(inspect.signature(T.BatchNorm2d.forward).parameters)[1:] == ["x"]              # the plain forward is as it was
    assert issubclass(T.ResidualBlock, T.Module)


def test_bad_arguments_are_refused_before_the_device_is_touched():
    # on a machine without a GPU nothing that needs the device could have succeeded: the refusal and its message come from the host
    import taper_amd as T
    from taper_amd._lib import host
    out = C.c_void_p()
    for args in ((0, 4, 1, 1), (4, 4, 0, 1), (4, 0, 1, 1), (-1, 4, 1, 1), (4, 4, -2, 1)):
        assert host.tp_residual_block_new(*args, C.byref(out)) != 0 and out.value is None, args
        assert "must be positive" in host.tp_last_error().decode()
    for kw in (dict(in_channels=0, out_channels=4), dict(in_channels=4, out_channels=4, stride=0)):
        with pytest.raises(T.TaperError, match="ResidualBlock: .*must be positive"):
            T.ResidualBlock(**kw)
    assert host.tp_residual_block_new(4, 4, 1, 1, None) != 0
    assert "null argument" in host.tp_last_error().decode()
