"""The exact pointwise convolution through the host (csrc/host: Tensor::conv2d's exact_pointwise, Conv2d, ResidualBlock's pointwise shortcut,
BottleneckBlock, the C ABI's flag word) on the GPU.

Conv2d(exact_pointwise=True), ResidualBlock.pointwise_shortcut(4, 8, 2), BottleneckBlock(8, 4, 16, 2) and BottleneckBlock(8, 4, 8, 1) against
float64 restatements (tests/conv_pw_ref.py's weight matrix, tests/conv_ref.py's 3x3 patches, tests/batchnorm_ref.py, tests/residual_ref.py)
through margins.check at the project's standing bar of 1e-4 of the tensor's scale; the blocks against the same layers composed by hand, on
bits; three Trainer steps eager and captured, on bits; and every refusal by name with the pool's in-use figure unchanged.  The host reads a
conv weight buffer [c_out][c_in][k][k] as the matrix [k k c_in][c_out] (weight_layout 0) in every exact convolution: the
restatements do the same."""
import ctypes as C
import gc
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import batchnorm_ref as BN
from tests import conv_pw_ref as PW
from tests import conv_ref, margins
from tests import residual_ref as RR
from tests.conv_s2_ref import dilate

pytestmark = pytest.mark.gpu
F = np.float32
BOUND = 1e-4      # README "Parity": of the tensor's scale


def _lib():
    from taper_amd._lib import hip
    return hip


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _same(name, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{name}: {bad.size} of {g.size} elements differ, the first at {bad[0]}"


def _pool_in_use(T):
    T.Device.sync()
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


# ---- float64 restatements.  Pointwise: the weight buffer read as [c_in][c_out]; 3x3 / pad 1 of stride 1 or 2: as [9 c_in][c_out]
def pw64(x, wt, s):
    return np.einsum("oc,nchw->nohw", PW.matrix(np.asarray(wt), 0), np.asarray(x, np.float64)[:, :, ::s, ::s])


def pw64_bwd(x, wt, gy, s):
    """-> (gw as it lies in memory [c_out, c_in, 1, 1], gx)"""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    gx = np.zeros(x.shape)
    gx[:, :, ::s, ::s] = np.einsum("oc,nohw->nchw", PW.matrix(np.asarray(wt), 0), gy)
    gw = np.einsum("nohw,nchw->co", gy, x[:, :, ::s, ::s])      # [c_in, c_out]: the buffer's own order under layout 0
    return gw.reshape(gy.shape[1], x.shape[1], 1, 1), gx


def conv64(x, wt, stride):
    return conv_ref._conv(np.asarray(x), conv_ref.weight_matrix(np.asarray(wt), 0), 1)[:, :, ::stride, ::stride]


def conv64_bwd(x, wt, gy, stride):
    """-> (gw as it lies in memory [c_out, c_in, 3, 3], gx)"""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    n, c_in, h, w = x.shape
    c_out = gy.shape[1]
    g = dilate(gy, h, w) if stride == 2 else gy
    std = conv_ref.weight_matrix(np.asarray(wt), 0).T.reshape(c_out, c_in, 3, 3)
    mir = np.ascontiguousarray(std[:, :, ::-1, ::-1].transpose(0, 2, 3, 1)).reshape(c_out * 9, c_in)
    gx = conv_ref._conv(g, mir, 1)
    p, _, _ = conv_ref.patches(x, 1)
    gw = p.T @ g.transpose(0, 2, 3, 1).reshape(-1, c_out)
    return gw.reshape(c_out, c_in, 3, 3), gx


# ---- 1. Conv2d(exact_pointwise=True) on float data ----
def _conv_case(T, s, relu):
    rng = np.random.default_rng(17 + s)
    shape = (3, 5, 9, 8)
    conv = (T.Conv2dReLU if relu else T.Conv2d)(5, 7, (1, 1), (s, s), (0, 0), seed=5, exact_pointwise=True)
    conv.parameters()[1].set_data(rng.standard_normal(7).astype(F) * 0.5)      # (the bias starts at zero)
    x = rng.standard_normal(shape).astype(F)
    oshape = (3, 7) + PW.out_hw(9, 8, s)
    g = rng.standard_normal(oshape).astype(F)
    return conv, x, g, shape, oshape


@pytest.mark.parametrize("relu", (False, True), ids=("plain", "relu"))
@pytest.mark.parametrize("s", (1, 2))
def test_conv2d_exact_pointwise_forward_and_full_backward(s, relu):
    """[3, 5, 9, 8] -> 7 with bias: y, and under full backward the weight, bias and input gradients of sum(y * g) + sum(x * x) -- the input has
    a second consumer whose gradient arrives first or second, so one of the two writes into the input's slot accumulates"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        conv, x, g, shape, oshape = _conv_case(T, s, relu)
        weight, bias = conv.parameters()
        wt, b = weight.data(), bias.data()
        pre = pw64(x, wt, s) + b.astype(np.float64)[None, :, None, None]
        y64 = np.maximum(pre, 0.0) if relu else pre
        gy = np.where(pre > 0, g.astype(np.float64), 0.0) if relu else g.astype(np.float64)
        gw64, gx64 = pw64_bwd(x, wt, gy, s)
        tx = T.Tensor(x, shape).requires_grad()
        y = conv.forward(tx)
        assert y.shape() == oshape
        ((y * T.Tensor(g, oshape)).sum() + (tx * tx).sum()).backward()
        if relu:
            assert (y.data() == 0).any() and (y.data() > 0).any(), "the case's ReLU cuts some outputs and keeps others"
        margins.check("y", y.data(), y64, BOUND)
        margins.check("weight_grad", weight.grad(), gw64, BOUND)
        margins.check("bias_grad", bias.grad(), gy.sum(axis=(0, 2, 3)), BOUND)
        margins.check("input_grad", tx.grad(), gx64 + 2.0 * x.astype(np.float64), BOUND)
        # the tensor op itself is the same convolution
        T.Tape.reset()
        op = T.Tensor(x, shape).conv2d_relu if relu else T.Tensor(x, shape).conv2d
        _same("conv2d_op", op(weight, bias, (s, s), (0, 0), exact_pointwise=True).data(), y.data())
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


def test_default_1x1_path_keeps_its_old_values():
    """the default 1x1 Conv2d on the same weights still runs the reference's reinterpretation: other values than the convolution's,
    the bits th_conv1x1_fwd(weight_layout 0) gives, and no weight or input gradient"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        conv, x, g, shape, oshape = _conv_case(T, 1, False)
        dflt = T.Conv2d(5, 7, (1, 1), (1, 1), (0, 0), seed=5)
        dflt.parameters()[1].set_data(conv.parameters()[1].data())
        _same("weights_from_the_same_seed", dflt.parameters()[0].data(), conv.parameters()[0].data())
        tx = T.Tensor(x, shape).requires_grad()
        yd = dflt.forward(tx)
        (yd * T.Tensor(g, oshape)).sum().backward()
        ye = conv.forward(T.Tensor(x, shape)).data()
        assert yd.shape() == oshape and not np.allclose(yd.data(), ye, atol=1e-3)
        assert tx.grad() is None, "the default 1x1 path has no input gradient"
        # its old values: the kernel entry point the default path has always called
        from taper_amd import hip
        ctx = hip.Ctx(0)
        dx, dw, db = ctx.upload(x), ctx.upload(dflt.parameters()[0].data()), ctx.upload(dflt.parameters()[1].data())
        dy = ctx.upload(np.zeros(oshape, F))
        ctx.call("th_conv1x1_fwd", dx, dw, db, dy, 3, 5, 9, 8, 7, 0, 0)
        _same("default_path_is_th_conv1x1_fwd", yd.data(), ctx.download(dy, oshape, F))
        ctx.close()
        with pytest.raises(T.TaperError, match="im2col_1x1 requires h_in == h_out"):
            T.Tensor(x, shape).conv2d(dflt.parameters()[0], None, (2, 2), (0, 0))
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


@pytest.mark.parametrize("s", (1, 2))
def test_conv2d_exact_pointwise_faithful_mode_bias_alone(s):
    """faithful mode (Q2): the chain stays cut at the conv -- the bias alone takes a gradient"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(False)
    conv, x, g, shape, oshape = _conv_case(T, s, True)
    weight, bias = conv.parameters()
    tx = T.Tensor(x, shape).requires_grad()
    y = conv.forward(tx)
    (y * T.Tensor(g, oshape)).sum().backward()
    pre = pw64(x, weight.data(), s) + bias.data().astype(np.float64)[None, :, None, None]
    margins.check("bias_grad", bias.grad(), np.where(pre > 0, g.astype(np.float64), 0.0).sum(axis=(0, 2, 3)), BOUND)
    assert weight.grad() is None and tx.grad() is None
    T.Tape.reset()


# ---- 2. the blocks ----
class _Layers:
    def parameters(self):
        return [p for l in self.layers for p in l.parameters()]

    def buffers(self):
        return [b for l in self.layers for b in l.buffers()]


class _ComposedResidual(_Layers):
    """ResidualBlock.pointwise_shortcut's layers by hand, with the block's seeds"""

    def __init__(self, T, cin, cout, stride, seed):
        self.conv1 = T.Conv2d(cin, cout, (3, 3), (stride, stride), (1, 1), bias=False, seed=seed, exact_stride=stride == 2)
        self.bn1 = T.BatchNorm2d(cout, fuse_relu=True)
        self.conv2 = T.Conv2d(cout, cout, (3, 3), (1, 1), (1, 1), bias=False, seed=seed + 1)
        self.bn2 = T.BatchNorm2d(cout, fuse_relu=True)
        self.conv3 = T.Conv2d(cin, cout, (1, 1), (stride, stride), (0, 0), bias=False, seed=seed + 2, exact_pointwise=True)
        self.bn3 = T.BatchNorm2d(cout)
        self.layers = [self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3]

    def forward(self, x):
        h = self.conv2.forward(self.bn1.forward(self.conv1.forward(x)))
        return self.bn2.forward_add(h, self.bn3.forward(self.conv3.forward(x)))


class _ComposedBottleneck(_Layers):
    """BottleneckBlock's layers by hand, with the block's seeds"""

    def __init__(self, T, cin, mid, cout, stride, seed):
        self.conv1 = T.Conv2d(cin, mid, (1, 1), (1, 1), (0, 0), bias=False, seed=seed, exact_pointwise=True)
        self.bn1 = T.BatchNorm2d(mid, fuse_relu=True)
        self.conv2 = T.Conv2d(mid, mid, (3, 3), (stride, stride), (1, 1), bias=False, seed=seed + 1, exact_stride=stride == 2)
        self.bn2 = T.BatchNorm2d(mid, fuse_relu=True)
        self.conv3 = T.Conv2d(mid, cout, (1, 1), (1, 1), (0, 0), bias=False, seed=seed + 2, exact_pointwise=True)
        self.bn3 = T.BatchNorm2d(cout, fuse_relu=True)
        self.layers = [self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3]
        self.proj = cin != cout or stride != 1
        if self.proj:
            self.conv4 = T.Conv2d(cin, cout, (1, 1), (stride, stride), (0, 0), bias=False, seed=seed + 3, exact_pointwise=True)
            self.bn4 = T.BatchNorm2d(cout)
            self.layers += [self.conv4, self.bn4]

    def forward(self, x):
        h = self.conv3.forward(self.bn2.forward(self.conv2.forward(self.bn1.forward(self.conv1.forward(x)))))
        return self.bn3.forward_add(h, self.bn4.forward(self.conv4.forward(x)) if self.proj else x)


def _zo(c):
    return np.zeros(c), np.ones(c)


def _residual64(x, P, k, stride, eps=1e-5):
    """the block with the pointwise shortcut in float64: y, the gradients of sum(y * k) for its nine parameters and the input, the BN records"""
    w1, g1, b1, w2, g2, b2, w3, g3, b3 = [np.asarray(p, np.float64) for p in P]
    z, o = _zo(len(g1))
    c1 = conv64(x, P[0], stride)
    f1 = BN.forward(c1, g1, b1, z, o, eps, 0.1, True, True)
    c2 = conv64(f1["y"], P[3], 1)
    c3 = pw64(x, P[6], stride)
    f3 = BN.forward(c3, g3, b3, z, o, eps, 0.1, True, False)
    f2 = RR.forward(c2, f3["y"], g2, b2, z, o, eps, 0.1, True, True)
    gc2, gr, gg2, gb2 = RR.backward(k, c2, g2, f2["save_mean"], f2["save_invstd"], f2["y"])
    gw2, ga1 = conv64_bwd(f1["y"], P[3], gc2, 1)
    gc1, gg1, gb1 = BN.backward(ga1, c1, g1, f1["save_mean"], f1["save_invstd"], f1["y"])
    gw1, gxa = conv64_bwd(x, P[0], gc1, stride)
    gc3, gg3, gb3 = BN.backward(gr, c3, g3, f3["save_mean"], f3["save_invstd"])
    gw3, gxb = pw64_bwd(x, P[6], gc3, stride)
    return f2["y"], [gw1, gg1, gb1, gw2, gg2, gb2, gw3, gg3, gb3, gxa + gxb], [f1, f2, f3]


def _bottleneck64(x, P, k, stride, eps=1e-5):
    """the bottleneck block in float64: y, the gradients of sum(y * k) for its 9 or 12 parameters and the input, the BN records in order"""
    proj = len(P) == 12
    Q = [np.asarray(p, np.float64) for p in P]
    g1, b1, g2, b2, g3, b3 = Q[1], Q[2], Q[4], Q[5], Q[7], Q[8]
    c1 = pw64(x, P[0], 1)
    f1 = BN.forward(c1, g1, b1, *_zo(len(g1)), eps, 0.1, True, True)
    c2 = conv64(f1["y"], P[3], stride)
    f2 = BN.forward(c2, g2, b2, *_zo(len(g2)), eps, 0.1, True, True)
    c3 = pw64(f2["y"], P[6], 1)
    if proj:
        g4, b4 = Q[10], Q[11]
        c4 = pw64(x, P[9], stride)
        f4 = BN.forward(c4, g4, b4, *_zo(len(g4)), eps, 0.1, True, False)
    res = f4["y"] if proj else np.asarray(x, np.float64)
    f3 = RR.forward(c3, res, g3, b3, *_zo(len(g3)), eps, 0.1, True, True)
    gc3, gr, gg3, gb3 = RR.backward(k, c3, g3, f3["save_mean"], f3["save_invstd"], f3["y"])
    gw3, ga2 = pw64_bwd(f2["y"], P[6], gc3, 1)
    gc2, gg2, gb2 = BN.backward(ga2, c2, g2, f2["save_mean"], f2["save_invstd"], f2["y"])
    gw2, ga1 = conv64_bwd(f1["y"], P[3], gc2, stride)
    gc1, gg1, gb1 = BN.backward(ga1, c1, g1, f1["save_mean"], f1["save_invstd"], f1["y"])
    gw1, gx = pw64_bwd(x, P[0], gc1, 1)
    grads, recs = [gw1, gg1, gb1, gw2, gg2, gb2, gw3, gg3, gb3], [f1, f2, f3]
    if proj:
        gc4, gg4, gb4 = BN.backward(gr, c4, g4, f4["save_mean"], f4["save_invstd"])
        gw4, gxb = pw64_bwd(x, P[9], gc4, stride)
        grads += [gw4, gg4, gb4]
        recs.append(f4)
        gx = gx + gxb
    else:
        gx = gx + gr
    return f3["y"], grads + [gx], recs


BLOCKS = {
    "residual_4_8_s2": (lambda T: T.ResidualBlock.pointwise_shortcut(4, 8, 2, seed=7), lambda T: _ComposedResidual(T, 4, 8, 2, 7),
                        lambda x, P, k: _residual64(x, P, k, 2), (6, 4, 9, 9), (6, 8, 5, 5),
                        [(8, 4, 3, 3), (8,), (8,), (8, 8, 3, 3), (8,), (8,), (8, 4, 1, 1), (8,), (8,)]),
    "bottleneck_8_4_16_s2": (lambda T: T.BottleneckBlock(8, 4, 16, 2, seed=7), lambda T: _ComposedBottleneck(T, 8, 4, 16, 2, 7),
                             lambda x, P, k: _bottleneck64(x, P, k, 2), (6, 8, 9, 9), (6, 16, 5, 5),
                             [(4, 8, 1, 1), (4,), (4,), (4, 4, 3, 3), (4,), (4,), (16, 4, 1, 1), (16,), (16,), (16, 8, 1, 1), (16,), (16,)]),
    "bottleneck_8_4_8_s1": (lambda T: T.BottleneckBlock(8, 4, 8, 1, seed=7), lambda T: _ComposedBottleneck(T, 8, 4, 8, 1, 7),
                            lambda x, P, k: _bottleneck64(x, P, k, 1), (6, 8, 9, 9), (6, 8, 9, 9),
                            [(4, 8, 1, 1), (4,), (4,), (4, 4, 3, 3), (4,), (4,), (8, 4, 1, 1), (8,), (8,)]),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_equals_the_composition_and_the_float64_block(name):
    """outputs, every parameter gradient, the input gradient and the running statistics: bit-identical to the same layers composed by hand from
    Conv2d, BatchNorm2d and forward_add with the same seeds, and within the bound of the float64 restatement"""
    import taper_amd as T
    make, compose, block64, shape, oshape, pshapes = BLOCKS[name]
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        rng = np.random.default_rng(31)
        x, k = rng.standard_normal(shape).astype(F), rng.standard_normal(oshape).astype(F)
        blk, ref = make(T), compose(T)
        assert [p.shape() for p in blk.parameters()] == pshapes
        assert len(blk.buffers()) == 2 * len(pshapes) // 3
        prng = np.random.default_rng(5)
        for p, q in zip(blk.parameters(), ref.parameters()):      # gamma, beta away from ones and zeros; same seeds: same conv weights
            if len(p.shape()) == 1:
                v = prng.uniform(0.5, 1.5, p.shape()).astype(F)
                p.set_data(v)
                q.set_data(v)
            else:
                _same("conv_weight_from_the_same_seed", p.data(), q.data())
        ys, xs = [], []
        for m in (blk, ref):
            T.Tape.reset()
            tx = T.Tensor(x, shape).requires_grad()
            y = m.forward(tx)
            (y * T.Tensor(k, oshape)).sum().backward()
            ys.append(y.data())
            xs.append(tx.grad())
        assert ys[0].shape == oshape
        _same("y", ys[0], ys[1])
        grads = [p.grad() for p in blk.parameters()] + [xs[0]]
        assert all(g is not None for g in grads), "every parameter and the input take gradients: " + str([g is not None for g in grads])
        for i, (p, q) in enumerate(zip(blk.parameters(), ref.parameters())):
            _same(f"param_{i}_grad", p.grad(), q.grad())
        _same("input_grad", xs[0], xs[1])
        for i, (a, b) in enumerate(zip(blk.buffers(), ref.buffers())):
            _same(f"buffer_{i}", a.data(), b.data())
        # the float64 restatement of the block
        y64, g64, recs = block64(x, [p.data() for p in blk.parameters()], k)
        margins.check("y", ys[0], y64, BOUND)
        assert len(grads) == len(g64)
        for i, (g, r) in enumerate(zip(grads, g64)):
            margins.check("input_grad" if i == len(g64) - 1 else f"param_{i}_grad", g, r, BOUND)
        for i, fr in enumerate(recs):
            margins.check(f"running_mean_{i}", blk.buffers()[2 * i].data(), fr["running_mean"], BOUND)
            margins.check(f"running_var_{i}", blk.buffers()[2 * i + 1].data(), fr["running_var"], BOUND)
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


def test_pointwise_shortcut_changes_nothing_with_an_identity_shortcut():
    import taper_amd as T
    T.Tape.reset()
    a, b = T.ResidualBlock.pointwise_shortcut(4, 4, 1, seed=3), T.ResidualBlock(4, 4, 1, seed=3)
    assert len(a.parameters()) == 6 and len(b.parameters()) == 6
    x = np.random.default_rng(1).standard_normal((2, 4, 6, 6)).astype(F)
    _same("y", a.forward(T.Tensor(x, (2, 4, 6, 6))).data(), b.forward(T.Tensor(x, (2, 4, 6, 6))).data())
    T.Tape.reset()


# ---- 3. training ----
def _train_model(T, seed=11):
    return T.Sequential([T.Conv2dReLU(1, 8, (3, 3), (1, 1), (1, 1), seed=seed), T.BottleneckBlock(8, 4, 16, 2, seed=seed + 1),
                         T.BottleneckBlock(16, 4, 16, 1, seed=seed + 5), T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(16, 10, seed=seed + 9)])


N_PARAMS, N_BUFFERS = 2 + 12 + 9 + 2, 8 + 6


def _state(model):
    return [p.data().copy() for p in model.parameters()], [b.data().copy() for b in model.buffers()]


def test_three_trainer_steps_eager_and_captured():
    """Stem conv, a downsampling and an identity bottleneck, global pool, Linear: three Adam steps under full backward.  The Trainer's loader
    feeds rows of 784 values, so both runs are on [8, 1, 28, 28]: eager and captured steps from the same start are bit-identical in every
    parameter, buffer and loss; every conv weight moves; on one fixed batch the loss is finite and lower after three steps"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        model = _train_model(T)
        assert len(model.parameters()) == N_PARAMS and len(model.buffers()) == N_BUFFERS
        opt = T.Adam(model.parameters(), 1e-2)
        loader = T.DataLoader(T.MNISTDataset.synthetic(24, 5), 8, False)
        tr = T.Trainer(model, opt, sample_shape=(1, 28, 28))
        path = Path(tempfile.mkdtemp()) / "adam.txt"
        tr.save_optimizer_state(path)
        start = _state(model)
        rg = tr.train_epoch_graph(loader)
        graph = _state(model)
        fresh = T.Trainer(model, opt, sample_shape=(1, 28, 28))
        for p, v in zip(model.parameters(), start[0]):
            p.set_data(v)
        for b, v in zip(model.buffers(), start[1]):
            b.set_data(v)
        fresh.load_optimizer_state(path)
        re = fresh.train_epoch(loader)
        eager = _state(model)
        assert len(rg["losses"]) == 3 and np.isfinite(rg["losses"]).all()
        np.testing.assert_array_equal(_bits(rg["losses"]), _bits(re["losses"]))
        for a, b in zip(graph[0] + graph[1], eager[0] + eager[1]):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        for i, (a, b) in enumerate(zip(start[0], eager[0])):
            if a.ndim == 4:
                assert not np.array_equal(a, b), f"conv weight {i} {a.shape} did not move"
        del tr, fresh, opt, model
        # one fixed batch, eagerly: the loss before the first step against the loss after the third
        rng = np.random.default_rng(2)
        x = rng.uniform(0, 1, (8, 1, 12, 12)).astype(F)
        lab = rng.integers(0, 10, 8).astype(F)
        T.Tape.reset()
        model = _train_model(T)
        opt = T.Adam(model.parameters(), 1e-2)
        tr = T.Trainer(model, opt)
        losses = [tr.train_step(T.Tensor(x, (8, 1, 12, 12)), T.Tensor(lab, (8,)))[0] for _ in range(3)]
        T.Tape.reset()
        after = float(T.cross_entropy_loss(model.forward(T.Tensor(x, (8, 1, 12, 12))), T.Tensor(lab, (8,))).data().reshape(-1)[0])
        print(f"losses before each step {losses}, after the third {after}")
        assert np.isfinite(losses + [after]).all() and after < losses[0], (losses, after)
        del tr, opt, model
    finally:
        T.set_full_backward(False)
        gc.collect()
        T.Tape.reset()


def test_machinery_covers_the_bottleneck_block():
    """train() / eval(), evaluate()'s flag restore, the checkpoint's buffers section and the data-parallel refusal reach a BottleneckBlock as
    they reach a ResidualBlock"""
    import taper_amd as T
    T.Tape.reset()
    lone = T.BatchNorm2d(16)
    model = T.Sequential([T.Conv2dReLU(1, 8, (3, 3), (1, 1), (1, 1), seed=2), T.BottleneckBlock(8, 4, 16, 2, seed=3), lone,
                          T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(16, 10, seed=4)])
    blk = model.layers[1]
    opt = T.Adam(model.parameters(), 1e-3)
    tr = T.Trainer(model, opt, sample_shape=(1, 28, 28))
    x8 = T.Tensor(np.random.default_rng(1).standard_normal((4, 8, 10, 10)).astype(F), (4, 8, 10, 10))

    def moves():
        before = [b.data().copy() for b in blk.buffers()]
        blk.forward(x8)
        changed = [not np.array_equal(a, b.data()) for a, b in zip(before, blk.buffers())]
        assert all(changed) or not any(changed), changed
        return changed[0]

    assert len(blk.buffers()) == 8
    model.eval()
    assert not moves(), "eval() reaches the block's four normalisations"
    model.train()
    assert moves(), "train() reaches the block's four normalisations"
    # evaluate() runs every layer on its running statistics and gives each its own flag back
    loader = T.DataLoader(T.MNISTDataset.synthetic(16, 5), 8, False)
    lone.eval()
    before = [b.data().copy() for b in model.buffers()]
    tr.evaluate(loader)
    assert all(np.array_equal(a, b.data()) for a, b in zip(before, model.buffers())), "evaluate() updates no running statistic"
    assert moves() and not lone.is_training()
    model.eval()
    tr.evaluate(loader)
    assert not moves() and not lone.is_training()
    model.train()
    assert lone.is_training()
    d = Path(tempfile.mkdtemp())
    tr.save_checkpoint(d / "bottleneck.txt")
    assert "buffers 10" in (d / "bottleneck.txt").read_text().splitlines()
    saved = _state(model)
    for t in model.parameters() + model.buffers():
        t.set_data(np.full(t.shape(), 7.0, F))
    tr.load_checkpoint(d / "bottleneck.txt")
    for a, b in zip(saved[0] + saved[1], model.parameters() + model.buffers()):
        assert np.array_equal(_bits(a), _bits(b.data()))
    comm = T.Communicator.loopback()
    with pytest.raises(T.TaperError, match="batch normalisation is not supported"):
        T.Trainer(model, opt, sample_shape=(1, 28, 28), comm=comm)
    del comm, tr, opt, model, blk, lone
    gc.collect()
    T.Tape.reset()


# ---- 4. refusals ----
def test_refusals_by_name_hold_nothing():
    import taper_amd as T
    from taper_amd._lib import host
    T.Tape.reset()
    x = T.Tensor(np.zeros((2, 4, 9, 9), F), (2, 4, 9, 9))
    w1, w3 = T.Tensor(np.zeros((8, 4, 1, 1), F), (8, 4, 1, 1)), T.Tensor(np.zeros((8, 4, 3, 3), F), (8, 4, 3, 3))
    good = T.Conv2d(4, 8, (1, 1), (2, 2), (0, 0), exact_pointwise=True)
    used = _pool_in_use(T)
    # a bare Conv2d, and the tensor op: every geometry other than 1x1 / stride (1, 1) or (2, 2) / padding (0, 0) / one group
    for kw, word in ((dict(stride=(3, 3)), "stride must be \\(1, 1\\) or \\(2, 2\\) \\(got \\(3, 3\\)\\)"),
                     (dict(stride=(2, 1)), "stride must be \\(1, 1\\) or \\(2, 2\\) \\(got \\(2, 1\\)\\)"),
                     (dict(padding=(1, 1)), "padding must be \\(0, 0\\) \\(got \\(1, 1\\)\\)"),
                     (dict(kernel_size=(3, 3)), "kernel must be 1x1 \\(got 3x3\\)"), (dict(groups=2), "groups must be 1")):
        args = dict(kernel_size=(1, 1), stride=(2, 2), padding=(0, 0))
        args.update(kw)
        with pytest.raises(T.TaperError, match="Conv2d exact_pointwise: .*" + word):
            T.Conv2d(4, 8, exact_pointwise=True, **args)
    with pytest.raises(T.TaperError, match="Conv2d: exact_stride and exact_pointwise exclude each other"):
        T.Conv2d(4, 8, (3, 3), (2, 2), (1, 1), exact_stride=True, exact_pointwise=True)
    for wt, s, p, d, word in ((w1, (3, 3), (0, 0), (1, 1), "stride must be \\(1, 1\\) or \\(2, 2\\)"), (w1, (1, 2), (0, 0), (1, 1), "stride must be"),
                              (w1, (2, 2), (1, 1), (1, 1), "padding must be \\(0, 0\\)"), (w3, (2, 2), (0, 0), (1, 1), "kernel must be 1x1 \\(got 3x3\\)"),
                              (w1, (1, 1), (0, 0), (2, 2), "dilation must be \\(1, 1\\)")):
        with pytest.raises(T.TaperError, match="conv2d exact_pointwise: .*" + word):
            x.conv2d(wt, None, s, p, d, exact_pointwise=True)
    with pytest.raises(T.TaperError, match="conv2d: exact_stride and exact_pointwise exclude each other"):
        x.conv2d(w1, None, (2, 2), (0, 0), exact_stride=True, exact_pointwise=True)
    # the blocks: strides 1 and 2 alone, positive sizes
    with pytest.raises(T.TaperError, match="ResidualBlock pointwise_shortcut: the stride must be 1 or 2 \\(got 3\\)"):
        T.ResidualBlock.pointwise_shortcut(4, 8, 3, exact_stride=False)
    with pytest.raises(T.TaperError, match="ResidualBlock (exact_stride|pointwise_shortcut): the stride must be 1 or 2 \\(got 3\\)"):
        T.ResidualBlock.pointwise_shortcut(4, 8, 3)
    with pytest.raises(T.TaperError, match="BottleneckBlock: the stride must be 1 or 2 \\(got 3\\)"):
        T.BottleneckBlock(8, 4, 16, 3)
    for bad in ((0, 4, 16, 1), (8, 0, 16, 1), (8, 4, 0, 1), (8, 4, 16, 0)):
        with pytest.raises(T.TaperError, match="BottleneckBlock: in_channels, mid_channels, out_channels and stride must be positive"):
            T.BottleneckBlock(*bad)
    # the flag word: 16 where it is known, unknown bits printed alone, 17 on a bare conv refused by name
    out = C.c_void_p()
    assert host.tp_conv2d_new_ex(4, 8, 1, 1, 2, 2, 0, 0, 1, 0, 1, 16, C.byref(out)) == 0 and out.value
    T.Module(out.value)
    out = C.c_void_p()
    assert host.tp_conv2d_ex(x._h, w1._h, None, 2, 2, 0, 0, 1, 1, 0, 16, C.byref(out)) == 0 and out.value
    assert T.Tensor(_h=out.value).shape() == (2, 8, 5, 5)
    for flags, n_params in ((16, 9), (17, 9)):
        out = C.c_void_p()
        assert host.tp_residual_block_new_ex(4, 8, 2, 1, flags, C.byref(out)) == 0 and out.value
        m = T.Module(out.value)
        assert [p.shape() for p in m.parameters()][6] == (8, 4, 1, 1) and len(m.parameters()) == n_params
        del m      # (what the accepted calls built goes back to the pool: the figure below is about the refused ones)
    out = C.c_void_p()
    assert host.tp_basic_block_new_ex(4, 8, 2, 1, 16, C.byref(out)) != 0 and out.value is None
    assert "tp_basic_block_new_ex: unknown flag bits 16 " in host.tp_last_error().decode()
    assert host.tp_basic_block_new_ex(4, 8, 2, 1, 17, C.byref(out)) != 0 and out.value is None
    assert "tp_basic_block_new_ex: unknown flag bits 16 " in host.tp_last_error().decode()
    assert host.tp_conv2d_new_ex(4, 8, 1, 1, 2, 2, 0, 0, 1, 0, 1, 17, C.byref(out)) != 0 and out.value is None
    assert "exact_stride and exact_pointwise exclude each other" in host.tp_last_error().decode()
    assert host.tp_conv2d_ex(x._h, w1._h, None, 2, 2, 0, 0, 1, 1, 0, 17, C.byref(out)) != 0 and out.value is None
    assert "exact_stride and exact_pointwise exclude each other" in host.tp_last_error().decode()
    for fn, call in (("tp_conv2d_new_ex", lambda f: host.tp_conv2d_new_ex(4, 8, 1, 1, 2, 2, 0, 0, 1, 0, 1, f, C.byref(out))),
                     ("tp_conv2d_ex", lambda f: host.tp_conv2d_ex(x._h, w1._h, None, 2, 2, 0, 0, 1, 1, 0, f, C.byref(out))),
                     ("tp_residual_block_new_ex", lambda f: host.tp_residual_block_new_ex(4, 8, 2, 1, f, C.byref(out)))):
        for flags, unknown in ((18, 2), (20, 4), (25, 8), (32, 32), (16 + 14, 14)):
            assert call(flags) != 0 and out.value is None
            assert f"{fn}: unknown flag bits {unknown} " in host.tp_last_error().decode(), host.tp_last_error()
    out = C.c_void_p()
    assert host.tp_bottleneck_block_new(8, 4, 16, 2, 1, None) != 0 and "tp_bottleneck_block_new: null argument" in host.tp_last_error().decode()
    assert host.tp_bottleneck_block_new(8, 4, 16, 5, 1, C.byref(out)) != 0 and out.value is None
    assert "BottleneckBlock: the stride must be 1 or 2 (got 5)" in host.tp_last_error().decode()
    gc.collect()
    assert _pool_in_use(T) == used
    # quantize: by name, before anything is allocated
    model = T.Sequential([good, T.ReLU(), T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(8, 10)])
    neck = T.Sequential([T.BottleneckBlock(4, 2, 8, 2), T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(8, 10)])
    calib = T.Tensor(np.random.default_rng(2).standard_normal((4, 4, 9, 9)).astype(F), (4, 4, 9, 9))
    used2 = _pool_in_use(T)
    for call in (lambda: model.quantize("int8"), lambda: model.quantize("float16"), lambda: model.quantize_static(calib),
                 lambda: model.quantize_static_conv(calib), lambda: model.quantize_static_chain(calib), lambda: good.quantize("int8")):
        with pytest.raises(T.TaperError, match="exact-pointwise Conv2d: quantized twins are a follow-up"):
            call()
        gc.collect()
    for call in (lambda: neck.quantize("int8"), lambda: neck.quantize_static(calib), lambda: neck.quantize_static_conv(calib)):
        with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
            call()
        gc.collect()
    assert _pool_in_use(T) == used2
    del model, neck, good, calib, x, w1, w3
    gc.collect()
    T.Tape.reset()
