"""BatchNorm2d / BasicBlock without a GPU: the float64 numpy restatement the GPU tests compare against (tests/batchnorm_ref.py) agrees
with the torch fixtures of tests/golden/make_golden_batchnorm.py; the libraries export the new entry points; the Python face exists with
its signatures; and what is refused on the host is refused before anything touches the device."""
import ctypes as C
import inspect
from pathlib import Path

import numpy as np
import pytest

from tests import batchnorm_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden"
TH = (("th_batchnorm2d_fwd", 15), ("th_batchnorm2d_bwd", 14), ("th_batchnorm2d_split", 3))      # (arguments behind ctx; split has none)
TP = (("tp_batchnorm2d_new", 5), ("tp_batchnorm2d_set_training", 2), ("tp_batchnorm2d_is_training", 2), ("tp_batchnorm2d_running_stats", 3),
      ("tp_batchnorm2d_set_running_stats", 3), ("tp_basic_block_new", 5), ("tp_module_num_buffers", 2), ("tp_module_buffer", 3),
      ("tp_module_set_training", 2))
BOUND = 1e-9   # of the tensor's scale: both sides are float64


def _close(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-300)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= BOUND, (name, err)


# ---- the restatement against torch ----
@pytest.mark.parametrize("name", ["batchnorm_2x5x3x3", "batchnorm_4x3x1x1"])
def test_reference_agrees_with_the_torch_fixture(name):
    g = np.load(GOLDEN / f"{name}.npz")
    c = g["gamma"].size
    rm, rv = np.zeros(c), np.ones(c)
    for k in range(3):   # three training forwards in a row: outputs and the running pair after each (unbiased variance)
        f = R.forward(g[f"x{k}"], g["gamma"], g["beta"], rm, rv, training=True)
        rm, rv = f["running_mean"], f["running_var"]
        _close(f"y{k}", f["y"], g[f"y{k}"])
        _close(f"rm{k}", rm, g[f"rm{k}"])
        _close(f"rv{k}", rv, g[f"rv{k}"])
    f = R.forward(g["xe"], g["gamma"], g["beta"], rm, rv, training=False)
    _close("ye", f["y"], g["ye"])
    assert np.array_equal(f["running_mean"], rm) and np.array_equal(f["running_var"], rv)
    for tag, relu in (("p", False), ("r", True)):
        f = R.forward(g[f"bx_{tag}"], g["gamma"], g["beta"], rm, rv, training=True, relu=relu)
        _close(f"by_{tag}", f["y"], g[f"by_{tag}"])
        gx, gg, gb = R.backward(g[f"bgy_{tag}"], g[f"bx_{tag}"], g["gamma"], f["save_mean"], f["save_invstd"], y=f["y"] if relu else None)
        _close(f"gx_{tag}", gx, g[f"gx_{tag}"])
        _close(f"gg_{tag}", gg, g[f"gg_{tag}"])
        _close(f"gb_{tag}", gb, g[f"gb_{tag}"])
    f = R.forward(g["bx_e"], g["gamma"], g["beta"], g["rm_e"], g["rv_e"], training=False)       # eval mode, affine pair still training
    gx, gg, gb = R.backward(g["bgy_e"], g["bx_e"], g["gamma"], f["save_mean"], f["save_invstd"], batch_stats=False)
    _close("gx_e", gx, g["gx_e"])
    _close("gg_e", gg, g["gg_e"])
    _close("gb_e", gb, g["gb_e"])


def trajectory_reference(g, steps=5, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """the fixture's model and Adam (torch defaults) restated on batchnorm_ref: -> (losses, final parameters, running pair)"""
    lr = float(g["lr"])
    p = [g["gamma0"].copy(), g["beta0"].copy(), g["w0"].copy(), g["b0"].copy()]
    m, v = [np.zeros_like(q) for q in p], [np.zeros_like(q) for q in p]
    rm, rv = np.zeros(3), np.ones(3)
    x, losses = g["x"], []
    for t in range(1, steps + 1):
        f = R.forward(x, p[0], p[1], rm, rv, training=True, relu=True)
        rm, rv = f["running_mean"], f["running_var"]
        h = f["y"].reshape(x.shape[0], -1)
        loss, gl = R.softmax_xent(h @ p[2].T + p[3], g["labels"])
        losses.append(loss)
        gh = (gl @ p[2]).reshape(x.shape)
        gx, gg, gb = R.backward(gh, x, p[0], f["save_mean"], f["save_invstd"], y=f["y"])
        grads = [gg, gb, gl.T @ h, gl.sum(axis=0)]
        for i, gr in enumerate(grads):
            m[i] = beta1 * m[i] + (1 - beta1) * gr
            v[i] = beta2 * v[i] + (1 - beta2) * gr * gr
            p[i] = p[i] - lr * (m[i] / (1 - beta1 ** t)) / (np.sqrt(v[i] / (1 - beta2 ** t)) + adam_eps)
    return np.array(losses), p, rm, rv


def test_reference_agrees_with_the_torch_trajectory():
    g = np.load(GOLDEN / "batchnorm_trajectory.npz")
    losses, p, rm, rv = trajectory_reference(g)
    _close("losses", losses, g["losses"])
    for name, got in zip(("gamma", "beta", "w", "b"), p):
        _close(name, got, g[name])
    _close("running_mean", rm, g["running_mean"])
    _close("running_var", rv, g["running_var"])


def test_reference_refuses_one_value_per_channel():
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        R.forward(np.zeros((1, 3, 1, 1)), np.ones(3), np.zeros(3), np.zeros(3), np.ones(3))


# ---- the boundary ----
def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS, hip
    for name, nargs in TH:
        assert name in HIP_PROTOS, name
        assert len(HIP_PROTOS[name][1]) == nargs + (0 if name.endswith("_split") else 1), name
        assert getattr(hip, name)
    assert {n for n in HIP_PROTOS if n.startswith("th_batchnorm")} == {n for n, _ in TH}
    fwd = HIP_PROTOS["th_batchnorm2d_fwd"][1]
    assert fwd[12] is C.c_float and fwd[13] is C.c_float and fwd[9] is C.c_int     # eps, momentum; n


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS, host
    for name, nargs in TP:
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name
        assert getattr(host, name)


def test_split_of_a_channel():
    """one workgroup per channel is not the grid when c is small: c = 2 with 200 704 elements per channel is shared among many"""
    from taper_amd._lib import hip
    assert hip.th_batchnorm2d_split(64, 2, 56 * 56) >= 32
    assert hip.th_batchnorm2d_split(2, 300, 4) == 1 and hip.th_batchnorm2d_split(4, 3, 1) == 1
    assert hip.th_batchnorm2d_split(0, 3, 4) == 0 and hip.th_batchnorm2d_split(2, -1, 4) == 0
    for n, c, hw in ((256, 32, 784), (64, 2, 3136), (8, 3, 256), (1 << 20, 1, 1)):
        s = hip.th_batchnorm2d_split(n, c, hw)
        assert 1 <= s <= 256 and (s == 1 or c * s <= 2048)


def test_python_face():
    import taper_amd as T
    assert {"BatchNorm2d", "BasicBlock"} <= set(T.__all__)
    sig = inspect.signature(T.BatchNorm2d.__init__)
    assert list(sig.parameters)[1:] == ["num_features", "eps", "momentum", "fuse_relu"]
    assert sig.parameters["eps"].default == 1e-5 and sig.parameters["momentum"].default == 0.1 and sig.parameters["fuse_relu"].default is False
    sig = inspect.signature(T.BasicBlock.__init__)
    assert list(sig.parameters)[1:] == ["in_channels", "out_channels", "stride", "seed"]
    assert sig.parameters["stride"].default == 1 and sig.parameters["seed"].default == 1
    for meth in ("train", "eval", "set_running_stats", "is_training"):
        assert callable(getattr(T.BatchNorm2d, meth))
    assert isinstance(T.BatchNorm2d.running_mean, property) and isinstance(T.BatchNorm2d.running_var, property)
    for meth in ("train", "eval", "buffers"):
        assert callable(getattr(T.Module, meth))
    assert T.Dropout.train is not T.Module.train and T.Dropout.eval is not T.Module.eval      # Dropout keeps its own


def test_bad_arguments_are_refused_before_the_device_is_touched():
    # on a machine without a GPU nothing that needs the device could have succeeded: the refusal and its message come from the host
    import taper_amd as T
    from taper_amd._lib import host
    for nf in (0, -3):
        with pytest.raises(T.TaperError, match="num_features must be positive"):
            T.BatchNorm2d(nf)
    for eps in (0.0, -1e-5, float("nan"), float("inf")):
        with pytest.raises(T.TaperError, match="eps must be finite and positive"):
            T.BatchNorm2d(3, eps=eps)
    for mom in (-0.1, 1.5, float("nan")):
        with pytest.raises(T.TaperError, match=r"momentum must be in \[0, 1\]"):
            T.BatchNorm2d(3, momentum=mom)
    out = C.c_void_p()
    assert host.tp_batchnorm2d_new(0, 1e-5, 0.1, 0, C.byref(out)) != 0 and out.value is None
    assert "num_features must be positive" in host.tp_last_error().decode()
    assert host.tp_basic_block_new(0, 4, 1, 1, C.byref(out)) != 0 and out.value is None
    assert "must be positive" in host.tp_last_error().decode()
    lin = T.ReLU()
    with pytest.raises(T.TaperError, match="not a BatchNorm2d module"):
        from taper_amd._lib import tp_check
        tp_check(host.tp_batchnorm2d_set_training(lin._h, 1), "set_training of a ReLU")
    assert lin.buffers() == []
    lin.eval()
    lin.train()
