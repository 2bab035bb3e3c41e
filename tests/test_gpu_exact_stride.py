"""The exact strided convolution through the host (csrc/host: Tensor::conv2d's exact_stride, Conv2d, BasicBlock, ResidualBlock, the C ABI's
*_ex entry points) on the GPU.

Conv2d(exact_stride=True) and ResidualBlock.exact_stride(4, 8, 2) against float64 restatements (tests/conv_ref.py's patches and
weight matrix, tests/batchnorm_ref.py, tests/residual_ref.py) through margins.check at the project's standing bar of 1e-4 of the tensor's
scale; the block against the same layers composed by hand, on bits; three Trainer steps eager and captured, on bits; and every refusal by
name with the pool's in-use figure unchanged.  The host reads a conv weight buffer [c_out][c_in][3][3] as the matrix [9 c_in][c_out]
(weight_layout 0) at every stride: the restatements do the same."""
import ctypes as C
import gc
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import batchnorm_ref as BN
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


# ---- float64 restatements: a 3x3 / pad 1 convolution of stride 1 or 2 with the weight buffer read as [9 c_in][c_out], and its gradients
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
    gw = p.T @ g.transpose(0, 2, 3, 1).reshape(-1, c_out)      # [9 c_in, c_out]: the buffer's own order under layout 0
    return gw.reshape(c_out, c_in, 3, 3), gx


# ---- 1. Conv2d(exact_stride=True) on float data ----
def _conv_case(T):
    rng = np.random.default_rng(17)
    shape = (3, 4, 9, 9)
    conv = T.Conv2dReLU(4, 8, (3, 3), (2, 2), (1, 1), seed=5, exact_stride=True)
    conv.parameters()[1].set_data(rng.standard_normal(8).astype(F) * 0.5)      # (the bias starts at zero)
    x = rng.standard_normal(shape).astype(F)
    g = rng.standard_normal((3, 8, 5, 5)).astype(F)
    return conv, x, g, shape


def test_conv2d_exact_stride_forward_and_full_backward():
    """[3, 4, 9, 9] -> 8 with bias and the fused ReLU: y, and under full backward the weight, bias and input gradients of sum(y * g)"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        conv, x, g, shape = _conv_case(T)
        weight, bias = conv.parameters()
        wt, b = weight.data(), bias.data()
        pre = conv64(x, wt, 2) + b.astype(np.float64)[None, :, None, None]
        y64 = np.maximum(pre, 0.0)
        gy = np.where(pre > 0, g.astype(np.float64), 0.0)
        gw64, gx64 = conv64_bwd(x, wt, gy, 2)
        tx = T.Tensor(x, shape).requires_grad()
        y = conv.forward(tx)
        assert y.shape() == (3, 8, 5, 5)
        (y * T.Tensor(g, (3, 8, 5, 5))).sum().backward()
        assert (y.data() == 0).any() and (y.data() > 0).any(), "the case's ReLU cuts some outputs and keeps others"
        margins.check("y", y.data(), y64, BOUND)
        margins.check("weight_grad", weight.grad(), gw64, BOUND)
        margins.check("bias_grad", bias.grad(), gy.sum(axis=(0, 2, 3)), BOUND)
        margins.check("input_grad", tx.grad(), gx64, BOUND)
        # the tensor op itself, without the ReLU, is the same convolution
        T.Tape.reset()
        y2 = T.Tensor(x, shape).conv2d(weight, bias, (2, 2), (1, 1), (1, 1), exact_stride=True)
        margins.check("y_conv2d_op", y2.data(), pre, BOUND)
        _same("conv2d_relu_op", T.Tensor(x, shape).conv2d_relu(weight, bias, (2, 2), (1, 1), exact_stride=True).data(), y.data())
        # and it is not what the default strided path computes (the reference's gather)
        dflt = T.Tensor(x, shape).conv2d(weight, bias, (2, 2), (1, 1), (1, 1)).data()
        assert dflt.shape == y2.data().shape and not np.allclose(dflt, y2.data(), atol=1e-3)
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


def test_conv2d_exact_stride_faithful_mode_bias_alone():
    """faithful mode (Q2): the chain stays cut at the conv, as at stride 1 -- the bias alone takes a gradient"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(False)
    conv, x, g, shape = _conv_case(T)
    weight, bias = conv.parameters()
    tx = T.Tensor(x, shape).requires_grad()
    y = conv.forward(tx)
    (y * T.Tensor(g, (3, 8, 5, 5))).sum().backward()
    pre = conv64(x, weight.data(), 2) + bias.data().astype(np.float64)[None, :, None, None]
    margins.check("bias_grad", bias.grad(), np.where(pre > 0, g.astype(np.float64), 0.0).sum(axis=(0, 2, 3)), BOUND)
    assert weight.grad() is None and tx.grad() is None
    T.Tape.reset()


# ---- 2. ResidualBlock.exact_stride(4, 8, 2) ----
class _Composed:
    """the block's layers by hand: Conv2d(exact_stride=True), BatchNorm2d and forward_add, with the block's seeds"""

    def __init__(self, T, cin, cout, seed):
        self.conv1 = T.Conv2d(cin, cout, (3, 3), (2, 2), (1, 1), bias=False, seed=seed, exact_stride=True)
        self.bn1 = T.BatchNorm2d(cout, fuse_relu=True)
        self.conv2 = T.Conv2d(cout, cout, (3, 3), (1, 1), (1, 1), bias=False, seed=seed + 1)
        self.bn2 = T.BatchNorm2d(cout, fuse_relu=True)
        self.conv3 = T.Conv2d(cin, cout, (3, 3), (2, 2), (1, 1), bias=False, seed=seed + 2, exact_stride=True)
        self.bn3 = T.BatchNorm2d(cout)
        self.layers = [self.conv1, self.bn1, self.conv2, self.bn2, self.conv3, self.bn3]

    def forward(self, x):
        h = self.conv2.forward(self.bn1.forward(self.conv1.forward(x)))
        return self.bn2.forward_add(h, self.bn3.forward(self.conv3.forward(x)))

    def parameters(self):
        return [p for l in self.layers for p in l.parameters()]

    def buffers(self):
        return [b for l in self.layers for b in l.buffers()]


def _block64(x, P, k, eps=1e-5):
    """the block in float64: y and the gradients of sum(y * k) for (conv1 w, g1, b1, conv2 w, g2, b2, projection w, g3, b3) and the input"""
    w1, g1, b1, w2, g2, b2, w3, g3, b3 = [np.asarray(p, np.float64) for p in P]
    c = len(g1)
    z, o = np.zeros(c), np.ones(c)
    c1 = conv64(x, P[0], 2)
    f1 = BN.forward(c1, g1, b1, z, o, eps, 0.1, True, True)
    c2 = conv64(f1["y"], P[3], 1)
    c3 = conv64(x, P[6], 2)
    f3 = BN.forward(c3, g3, b3, z, o, eps, 0.1, True, False)
    f2 = RR.forward(c2, f3["y"], g2, b2, z, o, eps, 0.1, True, True)
    gc2, gr, gg2, gb2 = RR.backward(k, c2, g2, f2["save_mean"], f2["save_invstd"], f2["y"])
    gw2, ga1 = conv64_bwd(f1["y"], P[3], gc2, 1)
    gc1, gg1, gb1 = BN.backward(ga1, c1, g1, f1["save_mean"], f1["save_invstd"], f1["y"])
    gw1, gxa = conv64_bwd(x, P[0], gc1, 2)
    gc3, gg3, gb3 = BN.backward(gr, c3, g3, f3["save_mean"], f3["save_invstd"])
    gw3, gxb = conv64_bwd(x, P[6], gc3, 2)
    return f2["y"], [gw1, gg1, gb1, gw2, gg2, gb2, gw3, gg3, gb3, gxa + gxb], [f1, f2, f3]


def test_exact_block_equals_the_composition_and_the_float64_block():
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        rng = np.random.default_rng(31)
        shape, oshape = (6, 4, 9, 9), (6, 8, 5, 5)
        x, k = rng.standard_normal(shape).astype(F), rng.standard_normal(oshape).astype(F)
        blk, ref, dflt = T.ResidualBlock.exact_stride(4, 8, 2, seed=7), _Composed(T, 4, 8, 7), T.ResidualBlock(4, 8, 2, seed=7)
        assert [p.shape() for p in blk.parameters()] == [(8, 4, 3, 3), (8,), (8,), (8, 8, 3, 3), (8,), (8,), (8, 4, 3, 3), (8,), (8,)]
        prng = np.random.default_rng(5)
        for p, q, d in zip(blk.parameters(), ref.parameters(), dflt.parameters()):      # gamma, beta away from ones and zeros; same seeds: same conv weights
            if len(p.shape()) == 1:
                v = prng.uniform(0.5, 1.5, p.shape()).astype(F)
                for t in (p, q, d):
                    t.set_data(v)
            else:
                _same("conv_weight_from_the_same_seed", p.data(), q.data())
                _same("conv_weight_from_the_same_seed", p.data(), d.data())
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
        assert all(g is not None for g in grads), "all nine parameters and the input take gradients: " + str([g is not None for g in grads])
        for i, (p, q) in enumerate(zip(blk.parameters(), ref.parameters())):
            _same(f"param_{i}_grad", p.grad(), q.grad())
        _same("input_grad", xs[0], xs[1])
        for i, (a, b) in enumerate(zip(blk.buffers(), ref.buffers())):
            _same(f"buffer_{i}", a.data(), b.data())
        T.Tape.reset()
        yd = dflt.forward(T.Tensor(x, shape)).data()
        assert yd.shape == oshape and not np.array_equal(_bits(yd), _bits(ys[0])), "the default block keeps the reference's strided gather"
        # the float64 restatement of the block
        y64, g64, f = _block64(x, [p.data() for p in blk.parameters()], k)
        margins.check("y", ys[0], y64, BOUND)
        for i, (g, r) in enumerate(zip(grads, g64)):
            margins.check("input_grad" if i == 9 else f"param_{i}_grad", g, r, BOUND)
        for i, (bn, fr) in enumerate(zip((0, 2, 4), f)):
            margins.check(f"running_mean_{i}", blk.buffers()[bn].data(), fr["running_mean"], BOUND)
            margins.check(f"running_var_{i}", blk.buffers()[bn + 1].data(), fr["running_var"], BOUND)
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


def test_basic_block_exact_stride_and_stride_1():
    """BasicBlock hands the flag to its conv at stride 2 (its weight then trains); at stride 1 the flag changes nothing"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        rng = np.random.default_rng(3)
        shape = (4, 3, 8, 8)
        x = rng.standard_normal(shape).astype(F)
        for stride, oshape in ((2, (4, 5, 4, 4)), (1, (4, 5, 8, 8))):
            k = rng.standard_normal(oshape).astype(F)
            res = []
            for exact in (True, False):
                T.Tape.reset()
                bb = (T.BasicBlock.exact_stride if exact else T.BasicBlock)(3, 5, stride, seed=4)
                tx = T.Tensor(x, shape).requires_grad()
                y = bb.forward(tx)
                (y * T.Tensor(k, oshape)).sum().backward()
                res.append((y.data(), bb.parameters()[0].grad(), tx.grad(), bb.parameters()[0].data()))
            if stride == 1:
                for a, b in zip(*res):
                    _same("stride_1_flag_changes_nothing", a, b)
            else:
                assert res[0][1] is not None and res[0][2] is not None and res[1][1] is None and res[1][2] is None
                c1 = conv64(x, res[0][3], 2) + 0.0      # (the conv's bias starts at zero)
                f1 = BN.forward(c1, np.ones(5), np.zeros(5), np.zeros(5), np.ones(5), 1e-5, 0.1, True, True)
                margins.check("y", res[0][0], f1["y"], BOUND)
                gc1 = BN.backward(k, c1, np.ones(5), f1["save_mean"], f1["save_invstd"], f1["y"])[0]
                gw, gx = conv64_bwd(x, res[0][3], gc1, 2)
                margins.check("weight_grad", res[0][1], gw, BOUND)
                margins.check("input_grad", res[0][2], gx, BOUND)
    finally:
        T.set_full_backward(False)
        T.Tape.reset()


# ---- 3. training ----
def _train_model(T, exact, seed=11):
    return T.Sequential([T.Conv2dReLU(1, 4, (3, 3), (1, 1), (1, 1), seed=seed), (T.ResidualBlock.exact_stride if exact else T.ResidualBlock)(4, 8, 2, seed=seed + 1),
                         T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(8, 10, seed=seed + 7)])


STRIDED = (2, 8)      # model.parameters(): the first conv's pair, then the block's nine -- conv1's weight and the projection's


def _state(model):
    return [p.data().copy() for p in model.parameters()], [b.data().copy() for b in model.buffers()]


def test_three_trainer_steps_eager_and_captured():
    """Three steps under full backward.  The Trainer's loader feeds rows of 784 values, so the captured path runs on [8, 1, 28, 28]: eager
    and captured steps from the same start are bit-identical, and both strided convs move.  Three eager train_step calls on [8, 1, 12, 12]
    move them too; the same model with the default block leaves them where they were (the behaviour that stays the default)."""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)
    try:
        model = _train_model(T, True)
        assert len(model.parameters()) == 2 + 9 + 2 and len(model.buffers()) == 6
        opt = T.Adam(model.parameters(), 1e-2)
        loader = T.DataLoader(T.MNISTDataset.synthetic(24, 5), 8, False)
        tr = T.Trainer(model, opt, sample_shape=(1, 28, 28), fuse_head=0)
        path = Path(tempfile.mkdtemp()) / "adam.txt"
        tr.save_optimizer_state(path)
        start = _state(model)
        rg = tr.train_epoch_graph(loader)
        graph = _state(model)
        fresh = T.Trainer(model, opt, sample_shape=(1, 28, 28), fuse_head=0)
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
        for i in STRIDED:
            assert start[0][i].shape == (8, 4, 3, 3) and not np.array_equal(start[0][i], eager[0][i]), f"strided conv weight {i} did not move"
        del tr, fresh, opt, model
        # the issue's own shape, eagerly; then the default block from the same seeds
        rng = np.random.default_rng(2)
        x12 = rng.uniform(0, 1, (8, 1, 12, 12)).astype(F)
        lab = rng.integers(0, 10, 8).astype(F)
        for exact in (True, False):
            T.Tape.reset()
            model = _train_model(T, exact)
            opt = T.Adam(model.parameters(), 1e-2)
            tr = T.Trainer(model, opt, fuse_head=0)
            before = _state(model)[0]
            losses = [tr.train_step(T.Tensor(x12, (8, 1, 12, 12)), T.Tensor(lab, (8,)))[0] for _ in range(3)]
            after = _state(model)[0]
            assert np.isfinite(losses).all()
            for i in STRIDED:
                moved = not np.array_equal(before[i], after[i])
                assert moved == exact, f"strided conv weight {i}: moved = {moved} with exact_stride = {exact}"
            assert not np.array_equal(before[5], after[5]), "conv2 (stride 1) trains in both"
            del tr, opt, model
    finally:
        T.set_full_backward(False)
        gc.collect()
        T.Tape.reset()


def test_machinery_covers_the_exact_block():
    """train() / eval(), the checkpoint and the data-parallel refusal reach an exact block as they reach the default one"""
    import taper_amd as T
    T.Tape.reset()
    model = _train_model(T, True)
    blk = model.layers[1]
    opt = T.Adam(model.parameters(), 1e-3)
    tr = T.Trainer(model, opt, sample_shape=(1, 28, 28))
    x4 = T.Tensor(np.random.default_rng(1).standard_normal((4, 4, 10, 10)).astype(F), (4, 4, 10, 10))
    before = [b.data().copy() for b in blk.buffers()]
    model.eval()
    blk.forward(x4)
    assert all(np.array_equal(a, b.data()) for a, b in zip(before, blk.buffers())), "eval() reaches the block's layers"
    model.train()
    blk.forward(x4)
    assert all(not np.array_equal(a, b.data()) for a, b in zip(before, blk.buffers())), "train() reaches the block's layers"
    d = Path(tempfile.mkdtemp())
    tr.save_checkpoint(d / "exact.txt")
    assert "buffers 6" in (d / "exact.txt").read_text().splitlines()
    saved = _state(model)
    for t in model.parameters() + model.buffers():
        t.set_data(np.full(t.shape(), 7.0, F))
    tr.load_checkpoint(d / "exact.txt")
    for a, b in zip(saved[0] + saved[1], model.parameters() + model.buffers()):
        assert np.array_equal(_bits(a), _bits(b.data()))
    comm = T.Communicator.loopback()
    with pytest.raises(T.TaperError, match="batch normalisation is not supported"):
        T.Trainer(model, opt, sample_shape=(1, 28, 28), comm=comm)
    del comm, tr, opt, model, blk
    gc.collect()
    T.Tape.reset()


# ---- 4. refusals ----
def test_refusals_by_name_hold_nothing():
    import taper_amd as T
    from taper_amd._lib import host
    T.Tape.reset()
    x = T.Tensor(np.zeros((2, 4, 9, 9), F), (2, 4, 9, 9))
    w3, w5 = T.Tensor(np.zeros((8, 4, 3, 3), F), (8, 4, 3, 3)), T.Tensor(np.zeros((8, 4, 5, 5), F), (8, 4, 5, 5))
    good = T.Conv2d(4, 8, (3, 3), (2, 2), (1, 1), exact_stride=True)
    used = _pool_in_use(T)
    # a bare Conv2d, and the tensor op: every geometry other than 3x3 / stride (2, 2) / padding (1, 1) / one group
    for kw, word in ((dict(stride=(1, 1)), "stride must be \\(2, 2\\)"), (dict(stride=(3, 3)), "stride must be \\(2, 2\\)"),
                     (dict(stride=(2, 1)), "stride must be \\(2, 2\\)"), (dict(padding=(0, 0)), "padding must be \\(1, 1\\)"),
                     (dict(kernel_size=(5, 5)), "kernel must be 3x3"), (dict(groups=2), "groups must be 1")):
        args = dict(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1))
        args.update(kw)
        with pytest.raises(T.TaperError, match="Conv2d exact_stride: .*" + word):
            T.Conv2d(4, 8, exact_stride=True, **args)
    for wt, s, p, d, word in ((w3, (1, 1), (1, 1), (1, 1), "stride must be \\(2, 2\\)"), (w3, (3, 3), (1, 1), (1, 1), "stride must be \\(2, 2\\)"),
                              (w3, (2, 2), (0, 0), (1, 1), "padding must be \\(1, 1\\)"), (w5, (2, 2), (1, 1), (1, 1), "kernel must be 3x3"),
                              (w3, (2, 2), (1, 1), (2, 2), "dilation must be \\(1, 1\\)")):
        with pytest.raises(T.TaperError, match="conv2d exact_stride: .*" + word):
            x.conv2d(wt, None, s, p, d, exact_stride=True)
    # the blocks: stride 1 is fine (the flag changes nothing), any other stride than 2 is refused by name
    for cls in (T.BasicBlock, T.ResidualBlock):
        with pytest.raises(T.TaperError, match=cls.__name__ + " exact_stride: the stride must be 1 or 2 \\(got 3\\)"):
            cls.exact_stride(4, 8, 3)
        cls.exact_stride(4, 8, 1)
    # unknown flag bits, each entry point by its own name
    out = C.c_void_p()
    assert host.tp_conv2d_new_ex(4, 8, 3, 3, 2, 2, 1, 1, 1, 0, 1, 2, C.byref(out)) != 0 and out.value is None
    assert "tp_conv2d_new_ex: unknown flag bits 2" in host.tp_last_error().decode()
    assert host.tp_basic_block_new_ex(4, 8, 2, 1, 5, C.byref(out)) != 0 and out.value is None
    assert "tp_basic_block_new_ex: unknown flag bits 4" in host.tp_last_error().decode()
    assert host.tp_residual_block_new_ex(4, 8, 2, 1, -2, C.byref(out)) != 0 and out.value is None
    assert "tp_residual_block_new_ex: unknown flag bits" in host.tp_last_error().decode()
    assert host.tp_conv2d_ex(x._h, w3._h, None, 2, 2, 1, 1, 1, 1, 0, 8, C.byref(out)) != 0 and out.value is None
    assert "tp_conv2d_ex: unknown flag bits 8" in host.tp_last_error().decode()
    assert _pool_in_use(T) == used
    # flags 0 is the old function
    assert host.tp_conv2d_ex(x._h, w3._h, None, 1, 1, 1, 1, 1, 1, 0, 0, C.byref(out)) == 0 and out.value
    assert T.Tensor(_h=out.value).shape() == (2, 8, 9, 9)
    # quantize: by name, before anything is allocated
    model = T.Sequential([good, T.ReLU(), T.AdaptiveAvgPool2d((1, 1)), T.Flatten(), T.Linear(8, 10)])
    calib = T.Tensor(np.random.default_rng(2).standard_normal((4, 4, 9, 9)).astype(F), (4, 4, 9, 9))
    used2 = _pool_in_use(T)
    for call in (lambda: model.quantize("int8"), lambda: model.quantize("float16"), lambda: model.quantize_static(calib), lambda: model.quantize_static_conv(calib),
                 lambda: good.quantize("int8"), lambda: T.Sequential([T.BasicBlock.exact_stride(4, 8, 2)]).quantize_static_conv(calib)):
        with pytest.raises(T.TaperError, match="exact-stride Conv2d: quantized twins are a follow-up"):
            call()
        gc.collect()
    assert _pool_in_use(T) == used2
    del model, good, calib, x, w3, w5
    gc.collect()
    T.Tape.reset()
