"""The residual tail and ResidualBlock on the GPU (csrc/batchnorm.hip: th_bn_residual_fwd / th_bn_residual_bwd; csrc/host/batchnorm.cpp).

Kernel level, on bits: the fused map is the plain call's value, then one add, then the ReLU, each rounded once, and the sums do not
involve the residual -- so y is np.maximum(y0 + r, floor) in float32 of the plain call's y0, every per-channel output is the plain
call's bit for bit, and gr is the masked gy itself.  Module level: the block against the same layers composed from public pieces
(bit-identical forward; gradients through margins.check at the project's 1e-4 of scale).  The float64 restatement the formulas are
held to is tests/residual_ref.py, pinned against torch in tests/test_residual_abi.py."""
import ctypes as C
import gc
import tempfile
from pathlib import Path

import numpy as np
import pytest

from tests import margins
from tests import residual_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
BOUND = 1e-4
EPS, MOM = 1e-5, 0.1
# shape -> th_batchnorm2d_split: one launch in single floats / float4s; split in float4s with a prefetched trip / in single floats; the
# column form in one launch and split, each with a partial channel tile; more items (2050 channels) than workgroups (2048)
SHAPES = {(2, 5, 3, 3): 1, (8, 3, 16, 16): 1, (64, 2, 56, 56): None, (40, 2, 15, 15): 3, (4, 3, 1, 1): 1, (200, 70, 1, 1): 6, (2, 2050, 2, 2): 1}
_ids = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _lib():
    from taper_amd._lib import hip
    return hip


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _same(name, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{name}: {bad.size} of {g.size} elements differ, the first at {bad[0]}: {np.asarray(got).reshape(-1)[bad[0]]!r} " \
                          f"against {np.asarray(want).reshape(-1)[bad[0]]!r}"


def _in_use(ctx):
    ctx.sync()
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(ctx.h, C.byref(r), C.byref(u)) == 0
    return u.value


_CASES = {}


def _case(shape):
    """finite random inputs of a shape, made once: x ~ N(m_c, s_c), r ~ N(0, 1), gy ~ N(0.5, 1), per-channel vectors, and the old
    contents the accumulate bits add to"""
    if shape in _CASES:
        return _CASES[shape]
    n, c, h, w = shape
    rng = np.random.default_rng(int(np.prod(shape)) * 16 + c)
    m, s = rng.uniform(-1, 1, c).reshape(1, c, 1, 1), rng.uniform(0.5, 2.0, c).reshape(1, c, 1, 1)
    d = dict(x=(rng.standard_normal(shape) * s + m).astype(F), r=rng.standard_normal(shape).astype(F),
             gy=(rng.standard_normal(shape) + 0.5).astype(F), gamma=rng.uniform(0.5, 1.5, c).astype(F), beta=rng.standard_normal(c).astype(F),
             rm=rng.uniform(-1, 1, c).astype(F), rv=rng.uniform(0.5, 2.0, c).astype(F), old_gx=rng.standard_normal(shape).astype(F),
             old_gr=rng.standard_normal(shape).astype(F), old_gg=rng.standard_normal(c).astype(F), old_gb=rng.standard_normal(c).astype(F))
    _CASES[shape] = d
    return d


class _Shifted:
    """`size` floats that begin `off` bytes into their allocation (off = 4: on no 16-byte boundary), holding `data` when given and
    NaN otherwise"""

    def __init__(self, ctx, size, off=0, data=None):
        self.ctx, self.size, self.floats = ctx, size, size + off // 4
        self.buf = ctx.empty(self.floats)
        self.ptr = self.buf.offset(off)
        if data is None:
            ctx.call("th_fill_f32", self.buf, float("nan"), self.floats)
        else:
            a = np.ascontiguousarray(data, F)
            assert a.size == size and _lib().th_memcpy_h2d(ctx.h, self.ptr, a.ctypes.data, a.nbytes) == 0

    def __int__(self):
        return self.ptr

    def get(self, shape):
        return self.ctx.download(self.ptr, shape)


class _Layer:
    """the device buffers of one layer and both forwards on them; `off`: where the plain call's y begins, `r_off`: where the residual
    (and, in the backward, gr) begins"""

    def __init__(self, ctx, shape, d, off=0, r_off=0):
        self.ctx, self.shape, self.d, self.off, self.r_off = ctx, shape, d, off, r_off
        self.n, self.c, self.hw = shape[0], shape[1], shape[2] * shape[3]
        self.size = int(np.prod(shape))
        self.x, self.gy = ctx.upload(d["x"]), ctx.upload(d["gy"])
        self.r = _Shifted(ctx, self.size, r_off, d["r"])
        self.gamma, self.beta = ctx.upload(d["gamma"]), ctx.upload(d["beta"])

    def _stats(self):
        return [_Shifted(self.ctx, self.c, 0, v) for v in (self.d["rm"], self.d["rv"])] + [_Shifted(self.ctx, self.c), _Shifted(self.ctx, self.c)]

    def forward(self, fused, training, relu):
        """-> (y, save_mean, save_invstd, running_mean, running_var); the fused call's y stays on the device as self.y"""
        rm, rv, sm, si = self._stats()
        y = _Shifted(self.ctx, self.size, 0 if fused else self.off)
        if fused:
            self.ctx.call("th_bn_residual_fwd", self.x, int(self.r), self.gamma, self.beta, int(y), int(rm), int(rv), int(sm), int(si), self.n,
                          self.c, self.hw, EPS, MOM, 1 if training else 0, 1 if relu else 0)
            self.y, self.sm, self.si = y, sm, si
        else:
            self.ctx.call("th_batchnorm2d_fwd", self.x, self.gamma, self.beta, int(y), int(rm), int(rv), int(sm), int(si), self.n, self.c,
                          self.hw, EPS, MOM, 1 if training else 0, 1 if relu else 0)
        return (y.get(self.shape),) + tuple(b.get((self.c,)) for b in (sm, si, rm, rv))

    def backward(self, fused, relu, batch_stats, acc=0, want_gx=True):
        """after a fused forward -> (gx, gr or None, ggamma, gbeta).  With accumulate bits the buffers start from the case's old
        contents, NaN otherwise; the plain call's gx begins `r_off` bytes in, so that it takes the same instance as the fused one"""
        d = self.d
        gx = _Shifted(self.ctx, self.size, 0 if fused else self.r_off, d["old_gx"] if acc & 1 else None)
        gr = _Shifted(self.ctx, self.size, self.r_off, d["old_gr"] if acc & 8 else None)
        gg = _Shifted(self.ctx, self.c, 0, d["old_gg"] if acc & 2 else None)
        gb = _Shifted(self.ctx, self.c, 0, d["old_gb"] if acc & 4 else None)
        y = int(self.y) if relu else None
        if fused:
            self.ctx.call("th_bn_residual_bwd", self.gy, self.x, y, self.gamma, int(self.sm), int(self.si), int(gx) if want_gx else None, int(gr),
                          int(gg), int(gb), self.n, self.c, self.hw, 1 if batch_stats else 0, acc)
        else:
            self.ctx.call("th_batchnorm2d_bwd", self.gy, self.x, y, self.gamma, int(self.sm), int(self.si), int(gx) if want_gx else None, int(gg),
                          int(gb), self.n, self.c, self.hw, 1 if batch_stats else 0, acc & 7)
        return gx.get(self.shape), gr.get(self.shape) if fused else None, gg.get((self.c,)), gb.get((self.c,))


def _check_forward(ctx, shape, off=0, r_off=0):
    d = _case(shape)
    lay = _Layer(ctx, shape, d, off, r_off)
    for training in (True, False):
        for relu in (False, True):
            tag = f"{'train' if training else 'eval'}_{'relu' if relu else 'plain'}"
            y0, sm0, si0, rm0, rv0 = lay.forward(False, training, False)
            y, sm, si, rm, rv = lay.forward(True, training, relu)
            assert np.isfinite(y).all()
            _same(f"y_{tag}", y, np.maximum(y0 + d["r"], F(0.0) if relu else F(-np.inf)))
            _same(f"save_mean_{tag}", sm, sm0)
            _same(f"save_invstd_{tag}", si, si0)
            _same(f"running_mean_{tag}", rm, rm0)
            _same(f"running_var_{tag}", rv, rv0)
            if not training:
                _same(f"running_mean_unchanged_{tag}", rm, d["rm"])
                _same(f"running_var_unchanged_{tag}", rv, d["rv"])
            _same(f"residual_unchanged_{tag}", lay.r.get(shape), d["r"])
            if relu:
                assert (y == 0).any() and (y > 0).any(), "the case's ReLU cuts some elements and keeps others"
    # the formulas: the float64 restatement, to the project's bound
    ref = R.forward(d["x"], d["r"], d["gamma"], d["beta"], d["rm"], d["rv"], EPS, MOM, True, True)
    y, sm, si, rm, rv = lay.forward(True, True, True)
    margins.check("y", y, ref["y"], BOUND)
    margins.check("running_var", rv, ref["running_var"], BOUND)


def _check_backward(ctx, shape, off=0, r_off=0):
    d = _case(shape)
    lay = _Layer(ctx, shape, d, off, r_off)
    for relu in (False, True):
        for batch_stats in (True, False):
            tag = f"{'relu' if relu else 'plain'}_{'batch' if batch_stats else 'running'}"
            y = lay.forward(True, batch_stats, relu)[0]
            want_gr = np.where(y > 0, d["gy"], F(0.0)).astype(F) if relu else d["gy"]
            plain = {}
            for acc in (0, 7, 15):
                gx0, _, gg0, gb0 = plain[acc] = lay.backward(False, relu, batch_stats, acc)
                gx, gr, gg, gb = lay.backward(True, relu, batch_stats, acc)
                assert not any(np.isnan(a).any() for a in (gx, gr, gg, gb)), f"{tag} acc {acc}: a NaN is left where an output belongs"
                _same(f"gx_{tag}_acc{acc}", gx, gx0)
                _same(f"ggamma_{tag}_acc{acc}", gg, gg0)
                _same(f"gbeta_{tag}_acc{acc}", gb, gb0)
                _same(f"gr_{tag}_acc{acc}", gr, d["old_gr"] + want_gr if acc & 8 else want_gr)
            # gx = null: the map still runs, for gr alone
            gx, gr, gg, gb = lay.backward(True, relu, batch_stats, 0, want_gx=False)
            assert np.isnan(gx).all(), "a null gx was written somewhere"
            _same(f"gr_without_gx_{tag}", gr, want_gr)
            _same(f"ggamma_without_gx_{tag}", gg, plain[0][2])
            _same(f"gbeta_without_gx_{tag}", gb, plain[0][3])
    # the formulas: the float64 restatement, to the project's bound
    f = R.forward(d["x"], d["r"], d["gamma"], d["beta"], d["rm"], d["rv"], EPS, MOM, True, True)
    lay.forward(True, True, True)
    gx, gr, gg, gb = lay.backward(True, True, True)
    rgx, rgr, rgg, rgb = R.backward(d["gy"], d["x"], d["gamma"], f["save_mean"], f["save_invstd"], f["y"])
    margins.check("gx", gx, rgx, BOUND)
    margins.check("ggamma", gg, rgg, BOUND)
    margins.check("gbeta", gb, rgb, BOUND)
    # (an element whose y rounds to the other side of 0 than the float64 y would move gr by a whole gy: none does in these cases)
    margins.check("gr", gr, rgr, BOUND)


# ---- 1. the kernels, every form ----
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_forward_is_the_plain_forward_plus_the_residual(ctx, shape):
    split = _lib().th_batchnorm2d_split(shape[0], shape[1], shape[2] * shape[3])
    assert split == SHAPES[shape] if SHAPES[shape] else split > 1
    _check_forward(ctx, shape)


@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_backward_is_the_plain_backward_plus_gr(ctx, shape):
    _check_backward(ctx, shape)


@pytest.mark.parametrize("shape", [(8, 3, 16, 16), (3, 2, 64, 64)], ids=["8x3x16x16_one_launch", "3x2x64x64_split"])
def test_an_unaligned_residual_takes_the_scalar_instance(ctx, shape):
    """only the residual (forward) and gr (backward) begin 4 bytes off a 16-byte boundary, on planes of whole float4s: the pointer list
    of the plan holds them, so the call takes the single-float instance -- whose sums group differently from the float4 instance's, and
    whose bits are those of a plain call pushed onto the single-float instance the same way (its y, its gx, 4 bytes off)"""
    _check_forward(ctx, shape, off=4, r_off=4)
    _check_backward(ctx, shape, off=4, r_off=4)


@pytest.mark.parametrize("shape", [(64, 2, 56, 56), (200, 70, 1, 1), (2, 5, 3, 3)], ids=["64x2x56x56", "200x70x1x1", "2x5x3x3"])
def test_two_runs_are_bit_identical(ctx, shape):
    d = _case(shape)
    runs = []
    for _ in range(2):
        lay = _Layer(ctx, shape, d)
        runs.append(lay.forward(True, True, True) + lay.backward(True, True, True, 0))
    for k, (a, b) in enumerate(zip(*runs)):
        _same(f"output_{k}", a, b)


def test_residual_may_be_the_input(ctx):
    """d_residual == d_x is allowed (both are only read): y = bn(x) + x"""
    shape = (8, 3, 16, 16)
    d = _case(shape)
    lay = _Layer(ctx, shape, d)
    y0 = lay.forward(False, True, False)[0]
    rm, rv, sm, si = lay._stats()
    y = _Shifted(ctx, lay.size)
    ctx.call("th_bn_residual_fwd", lay.x, lay.x, lay.gamma, lay.beta, int(y), int(rm), int(rv), int(sm), int(si), lay.n, lay.c, lay.hw, EPS, MOM, 1, 0)
    _same("y", y.get(shape), y0 + d["x"])


# ---- 2. refusals ----
def test_kernel_refusals_name_their_entry_point_and_touch_nothing(ctx):
    L = _lib()
    n, c, hw = 2, 3, 4
    rng = np.random.default_rng(0)
    x, gy, r = (ctx.upload(rng.standard_normal(n * c * hw).astype(F)) for _ in range(3))
    gamma, beta = ctx.upload(np.ones(c, F)), ctx.upload(np.zeros(c, F))
    sizes = dict(y=n * c * hw, rm=c, rv=c, sm=c, si=c, gx=n * c * hw, gr=n * c * hw, gg=c, gb=c)
    outs = {k: ctx.empty(sz) for k, sz in sizes.items()}
    for k, b in outs.items():
        ctx.call("th_fill_f32", b, float("nan"), sizes[k])
    P = {k: int(v) for k, v in outs.items()}
    X, GY, RES, G, B = int(x), int(gy), int(r), int(gamma), int(beta)
    before = _in_use(ctx)

    def fwd(x=X, r=RES, gamma=G, beta=B, y=P["y"], rm=P["rm"], rv=P["rv"], sm=P["sm"], si=P["si"], n=n, c=c, hw=hw, eps=EPS, mom=MOM, training=1):
        return L.th_bn_residual_fwd(ctx.h, x, r, gamma, beta, y, rm, rv, sm, si, n, c, hw, eps, mom, training, 0)

    def bwd(gy=GY, x=X, gamma=G, sm=P["sm"], si=P["si"], gx=P["gx"], gr=P["gr"], gg=P["gg"], gb=P["gb"], n=n, c=c, hw=hw, acc=0):
        return L.th_bn_residual_bwd(ctx.h, gy, x, None, gamma, sm, si, gx, gr, gg, gb, n, c, hw, 1, acc)

    def refused(rc, entry, text=None):
        msg = L.th_last_error().decode()
        assert rc != 0 and entry in msg and (text is None or text in msg), (rc, msg)

    refused(fwd(r=None), "th_bn_residual_fwd", "null argument")
    refused(fwd(r=P["y"]), "th_bn_residual_fwd", "d_residual may not be d_y")
    for bad in (dict(n=0), dict(n=-1), dict(c=0), dict(c=-2), dict(hw=0), dict(hw=-4), dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None),
                dict(rm=None), dict(rv=None), dict(sm=None), dict(si=None), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")),
                dict(eps=float("inf")), dict(mom=-0.5), dict(mom=1.5), dict(mom=float("nan"))):
        refused(fwd(**bad), "th_bn_residual_fwd")
    refused(fwd(n=1, hw=1), "th_bn_residual_fwd", "Expected more than 1 value per channel when training")
    refused(bwd(gr=None), "th_bn_residual_bwd", "null argument")
    refused(bwd(gr=P["gx"]), "th_bn_residual_bwd", "d_gr may not be d_gx")
    for bad in (dict(n=0), dict(c=-1), dict(hw=0), dict(gy=None), dict(x=None), dict(gamma=None), dict(sm=None), dict(si=None), dict(gg=None),
                dict(gb=None), dict(acc=16), dict(acc=-1)):
        refused(bwd(**bad), "th_bn_residual_bwd")
    assert _in_use(ctx) == before
    for k, b in outs.items():
        assert np.isnan(ctx.download(b, (sizes[k],))).all(), f"a refused call wrote to {k}"
    ctx.call("th_fill_f32", outs["rm"], 0.0, c)                    # the context is still usable
    ctx.call("th_fill_f32", outs["rv"], 1.0, c)
    assert fwd() == 0 and bwd() == 0 and bwd(gx=None) == 0
    assert all(np.isfinite(ctx.download(b, (sizes[k],))).all() for k, b in outs.items())
    assert _in_use(ctx) == before


def test_forward_add_refusals():
    import taper_amd as T
    T.Tape.reset()
    bn = T.BatchNorm2d(3)
    x = T.Tensor(np.zeros((2, 3, 2, 2), F), (2, 3, 2, 2))
    with pytest.raises(T.TaperError, match="BatchNorm2d::forward_add: the residual's shape differs"):
        bn.forward_add(x, T.Tensor(np.zeros((2, 3, 2, 1), F), (2, 3, 2, 1)))
    with pytest.raises(T.TaperError, match="BatchNorm2d::forward_add: the residual's shape differs"):
        bn.forward_add(x, T.Tensor(np.zeros((2, 3, 4), F), (2, 3, 4)))
    with pytest.raises(T.TaperError, match="BatchNorm2d::forward_add: the residual shares its storage with the input"):
        bn.forward_add(x, x)
    with pytest.raises(T.TaperError, match="BatchNorm2d::forward_add: .*channels"):
        bn.forward_add(T.Tensor(np.zeros((2, 4, 2, 2), F), (2, 4, 2, 2)), T.Tensor(np.zeros((2, 4, 2, 2), F), (2, 4, 2, 2)))
    with pytest.raises(T.TaperError, match="not a BatchNorm2d module"):
        T.BatchNorm2d.forward_add(T.ReLU(), x, T.Tensor(np.zeros((2, 3, 2, 2), F), (2, 3, 2, 2)))
    assert np.array_equal(bn.running_mean, np.zeros(3, F)) and np.array_equal(bn.running_var, np.ones(3, F))
    T.Tape.reset()


# ---- 3. the tape op ----
@pytest.mark.parametrize("fuse_relu", [False, True], ids=["plain", "relu"])
def test_forward_add_gradients(fuse_relu):
    """one node, four gradients, against the float64 restatement; a residual that takes no gradient leaves the others' bits alone"""
    import taper_amd as T
    rng = np.random.default_rng(8)
    shape = (4, 3, 5, 5)
    x, r, k = ((rng.standard_normal(shape) * s + m).astype(F) for s, m in ((1.5, 0.4), (1.0, 0.0), (1.0, 0.0)))
    gamma, beta = rng.uniform(0.5, 1.5, 3).astype(F), rng.standard_normal(3).astype(F)
    f = R.forward(x, r, gamma, beta, np.zeros(3), np.ones(3), EPS, MOM, True, fuse_relu)
    rgx, rgr, rgg, rgb = R.backward(k, x, gamma, f["save_mean"], f["save_invstd"], f["y"] if fuse_relu else None)
    kept = []
    for needs in (True, False):
        T.Tape.reset()
        bn = T.BatchNorm2d(3, fuse_relu=fuse_relu)
        bn.gamma.set_data(gamma)
        bn.beta.set_data(beta)
        tx, tr = T.Tensor(x, shape).requires_grad(), T.Tensor(r, shape)
        if needs:
            tr = tr.requires_grad()
        n0 = T.Tape.len()
        y = bn.forward_add(tx, tr)
        assert T.Tape.len() == n0 + 1, "forward_add is one tape node"
        (y * T.Tensor(k, shape)).sum().backward()
        margins.check("y", y.data(), f["y"], BOUND)
        margins.check("x_grad", tx.grad(), rgx, BOUND)
        if needs:
            margins.check("residual_grad", tr.grad(), rgr, BOUND)
        else:
            assert tr.grad() is None
        margins.check("gamma_grad", bn.gamma.grad(), rgg, BOUND)
        margins.check("beta_grad", bn.beta.grad(), rgb, BOUND)
        margins.check("running_var", bn.running_var, f["running_var"], BOUND)
        kept.append((tx.grad(), bn.gamma.grad(), bn.beta.grad()))
    for a, b in zip(*kept):
        _same("with_and_without_the_residual's_gradient", a, b)
    T.Tape.reset()


# ---- 4. the block against the same layers from public pieces ----
class _Composed:
    """ResidualBlock's layers from Conv2d, BatchNorm2d, Tensor.__add__ and relu, with the block's seeds"""

    def __init__(self, T, cin, cout, stride=1, seed=1):
        self.conv1 = T.Conv2d(cin, cout, (3, 3), (stride, stride), (1, 1), bias=False, seed=seed)
        self.bn1 = T.BatchNorm2d(cout, fuse_relu=True)
        self.conv2 = T.Conv2d(cout, cout, (3, 3), (1, 1), (1, 1), bias=False, seed=seed + 1)
        self.bn2 = T.BatchNorm2d(cout)
        self.layers = [self.conv1, self.bn1, self.conv2, self.bn2]
        self.proj = cin != cout or stride != 1
        if self.proj:
            self.conv3 = T.Conv2d(cin, cout, (3, 3), (stride, stride), (1, 1), bias=False, seed=seed + 2)
            self.bn3 = T.BatchNorm2d(cout)
            self.layers += [self.conv3, self.bn3]

    def forward(self, x):
        h = self.bn2.forward(self.conv2.forward(self.bn1.forward(self.conv1.forward(x))))
        s = self.bn3.forward(self.conv3.forward(x)) if self.proj else x
        return (h + s).relu()

    def parameters(self):
        return [p for l in self.layers for p in l.parameters()]

    def buffers(self):
        return [b for l in self.layers for b in l.buffers()]

    def train(self):
        for l in self.layers:
            l.train()

    def eval(self):
        for l in self.layers:
            l.eval()


BLOCKS = {"identity_4_4": (4, 4, 1), "projection_4_8_stride_2": (4, 8, 2)}


def _perturb(params, other, seed):
    """gamma and beta away from ones and zeros, the same in both models (the conv weights already agree: same seeds)"""
    rng = np.random.default_rng(seed)
    for p, q in zip(params, other):
        assert p.shape() == q.shape()
        if len(p.shape()) == 1:
            v = rng.uniform(0.5, 1.5, p.shape()).astype(F)
            p.set_data(v)
            q.set_data(v)
        else:
            _same("conv_weight_from_the_same_seed", p.data(), q.data())


def _grads_agree(name, got, want):
    """both None (a tensor the tape never reaches: a conv weight in faithful mode, a strided conv's in either), or within the bound"""
    assert (got is None) == (want is None), f"{name}: one side has a gradient, the other has none"
    if want is not None:
        margins.check(name, got, want, BOUND)


@pytest.mark.parametrize("full", [True, False], ids=["full_backward", "faithful"])
@pytest.mark.parametrize("which", list(BLOCKS), ids=list(BLOCKS))
def test_block_equals_the_composition(which, full):
    """full_backward: the conv weights (of the stride-1 convs) and the input through conv1 take gradients, so the identity block's
    input gets its gradient from both consumers; faithful mode (the default, quirk Q2) cuts the chain at every conv, which leaves the
    normalisations' pairs and the skip connection -- and a main branch whose input takes no gradient (gx null, gr alone)"""
    import taper_amd as T
    cin, cout, stride = BLOCKS[which]
    T.Tape.reset()
    T.set_full_backward(full)
    rng = np.random.default_rng(31)
    shape = (6, 4, 9, 9)
    x = rng.standard_normal(shape).astype(F)
    blk, ref = T.ResidualBlock(cin, cout, stride, seed=7), _Composed(T, cin, cout, stride, seed=7)
    want_shapes = [(cout, cin, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)] + ([(cout, cin, 3, 3), (cout,), (cout,)] if ref.proj else [])
    assert [p.shape() for p in blk.parameters()] == want_shapes
    assert [b.shape() for b in blk.buffers()] == [(cout,)] * (6 if ref.proj else 4)
    _perturb(blk.parameters(), ref.parameters(), 5)
    oshape = (6, cout, 9 if stride == 1 else 5, 9 if stride == 1 else 5)
    k = rng.standard_normal(oshape).astype(F)
    grads = []
    for rep in range(2):                                    # the second pass adds to every gradient the first one left
        ys, xs = [], []
        for m in (blk, ref):
            T.Tape.reset()
            tx = T.Tensor(x, shape).requires_grad()
            if rep and grads[0][-1] is not None:
                tx.set_grad(grads[0][-1])           # (a new input tensor each pass: it starts from the gradient the first pass left)
            y = m.forward(tx)
            (y * T.Tensor(k, oshape)).sum().backward()
            ys.append(y.data())
            xs.append(tx.grad())
        assert ys[0].shape == oshape
        _same(f"y_training_{rep}", ys[0], ys[1])
        for i, (p, q) in enumerate(zip(blk.parameters(), ref.parameters())):
            _grads_agree(f"param_{i}_grad", p.grad(), q.grad())
        _grads_agree("input_grad", xs[0], xs[1])
        for i, (a, b) in enumerate(zip(blk.buffers(), ref.buffers())):
            margins.check(f"buffer_{i}", a.data(), b.data(), BOUND)
        grads.append([p.grad() for p in blk.parameters()] + [xs[0]])
    with_grad = [i for i, g in enumerate(grads[0]) if g is not None]
    want = {True: {"identity_4_4": [0, 1, 2, 3, 4, 5, 6], "projection_4_8_stride_2": [1, 2, 3, 4, 5, 7, 8]},      # (strided convs: no gradient)
            False: {"identity_4_4": [4, 5, 6], "projection_4_8_stride_2": [4, 5, 7, 8]}}[full][which]
    assert with_grad == want, f"the tensors with a gradient (the input is the last index): {with_grad}"
    for i in with_grad:
        margins.check(f"gradient_{i}_doubles_without_zero_grad", grads[1][i], 2.0 * grads[0][i].astype(np.float64), BOUND)
    blk.eval()
    ref.eval()
    before = [b.data().copy() for b in blk.buffers()]
    T.Tape.reset()
    _same("y_eval", blk.forward(T.Tensor(x, shape)).data(), ref.forward(T.Tensor(x, shape)).data())
    for a, b in zip(before, blk.buffers()):
        _same("eval_mode_leaves_the_running_pair", b.data(), a)
    blk.train()
    blk.forward(T.Tensor(x, shape))
    assert not np.array_equal(before[0], blk.buffers()[0].data()), "train() reaches the block's layers"
    T.Tape.reset()


# ---- 5. three Adam steps ----
def test_three_adam_steps_follow_the_composition():
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(True)          # (the stride-1 conv weights train too)
    lr = 1e-2
    rng = np.random.default_rng(41)
    shape = (6, 4, 9, 9)
    x, labels = T.Tensor(rng.standard_normal(shape).astype(F), shape), T.Tensor(rng.integers(0, 5, 6).astype(F), (6,))

    def run(make):
        b1, b2, lin = make(4, 4, 1, 21), make(4, 8, 2, 31), T.Linear(200, 5, seed=9)
        params = b1.parameters() + b2.parameters() + lin.parameters()
        opt = T.Adam(params, lr)
        losses = []
        for _ in range(3):
            T.Tape.reset()
            loss = T.cross_entropy_loss(lin.forward(b2.forward(b1.forward(x)).flatten(1)), labels)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(float(loss.data()[0]))
        T.Tape.reset()
        return losses, [p.data() for p in params], [b.data() for b in b1.buffers() + b2.buffers()]

    got = run(lambda i, o, s, seed: T.ResidualBlock(i, o, s, seed=seed))
    ref = run(lambda i, o, s, seed: _Composed(T, i, o, s, seed=seed))
    for i, (a, b) in enumerate(zip(got[0], ref[0])):
        print(f"step {i}: loss {a:.7f} composed {b:.7f}")
        assert abs(a - b) <= 1e-4 * abs(b), (i, a, b)
    assert got[0][2] < got[0][0], "three steps lower the loss"
    for i, (p, q) in enumerate(zip(got[1], ref[1])):
        margins.check(f"param_{i}", p.reshape(-1), q.reshape(-1), 2e-2, lr=lr)
    for i, (a, b) in enumerate(zip(got[2], ref[2])):
        margins.check(f"buffer_{i}", a, b, BOUND)


# ---- 6. Trainer ----
def _trainer_model(T, seed=11):
    return T.Sequential([T.Conv2d(1, 4, (3, 3), (1, 1), (1, 1), seed=seed), T.ReLU(), T.ResidualBlock(4, 4, seed=seed + 1),
                         T.ResidualBlock(4, 8, 2, seed=seed + 4), T.AdaptiveAvgPool2d.global_(), T.Flatten(), T.Linear(8, 10, seed=seed + 7)])


def _state(model):
    return [p.data().copy() for p in model.parameters()], [b.data().copy() for b in model.buffers()]


def _restore(model, tr, state, path):
    for p, v in zip(model.parameters(), state[0]):
        p.set_data(v)
    for b, v in zip(model.buffers(), state[1]):
        b.set_data(v)
    tr.load_optimizer_state(path)


def _pool_in_use(T):
    T.Device.sync()
    r, u = C.c_size_t(), C.c_size_t()
    assert _lib().th_pool_stats(T.Device.ctx_handle(), C.byref(r), C.byref(u)) == 0
    return u.value


@pytest.mark.parametrize("full", [False, True], ids=["faithful", "full_backward"])
def test_trainer_graph_epoch_equals_eager_epoch(full):
    """the same epoch from the same start, captured and eager, with the classifier's fused forms off: the very same launches, so losses,
    parameters and running pairs are bit-identical"""
    import taper_amd as T
    T.Tape.reset()
    T.set_full_backward(full)
    model = _trainer_model(T)
    assert len(model.parameters()) == 2 + 6 + 9 + 2 and len(model.buffers()) == 4 + 6
    opt = T.Adam(model.parameters(), 1e-3)
    loader = T.DataLoader(T.MNISTDataset.synthetic(128, 5), 32, False)
    tr = T.Trainer(model, opt, sample_shape=(1, 28, 28), fuse_head=0)
    path = Path(tempfile.mkdtemp()) / "adam.txt"
    tr.save_optimizer_state(path)
    start = _state(model)
    rg = tr.train_epoch_graph(loader)
    graph = _state(model)
    for k in range(0, 10, 2):
        assert not np.array_equal(graph[1][k], start[1][k]), f"the captured steps did not update running mean {k // 2}"
    fresh = T.Trainer(model, opt, sample_shape=(1, 28, 28), fuse_head=0)
    _restore(model, fresh, start, path)
    re = fresh.train_epoch(loader)
    eager = _state(model)
    assert len(rg["losses"]) == 4 and np.isfinite(rg["losses"]).all()
    np.testing.assert_array_equal(_bits(rg["losses"]), _bits(re["losses"]))
    for a, b in zip(graph[0] + graph[1], eager[0] + eager[1]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert any(not np.array_equal(a, b) for a, b in zip(start[0], eager[0]))
    T.Tape.reset()


def test_trainer_modes_checkpoint_and_refusals():
    import taper_amd as T
    T.Tape.reset()
    model = _trainer_model(T)
    blk = model.layers[2]
    opt = T.Adam(model.parameters(), 1e-3)
    loader = T.DataLoader(T.MNISTDataset.synthetic(128, 6), 32, False)
    tr = T.Trainer(model, opt, sample_shape=(1, 28, 28))
    tr.train_epoch_graph(loader)
    # evaluate: running statistics for the duration, every layer's flag and running pair as it found them
    before = [b.data().copy() for b in model.buffers()]
    x4 = T.Tensor(np.random.default_rng(1).standard_normal((4, 4, 28, 28)).astype(F), (4, 4, 28, 28))
    for mode in (False, True):
        (model.train if mode else model.eval)()
        r = tr.evaluate(loader)
        assert np.isfinite(r["avg_loss"])
        for a, b in zip(before, model.buffers()):
            assert np.array_equal(_bits(a), _bits(b.data())), "evaluate changed the running statistics"
        blk.forward(x4)                                   # the block's first two layers show the mode they were left in
        changed = [not np.array_equal(a, b.data()) for a, b in zip(before[:4], blk.buffers())]
        assert all(changed) if mode else not any(changed), f"evaluate left a layer in the other mode (training = {mode}: {changed})"
        for b, v in zip(model.buffers(), before):
            b.set_data(v)
    T.Tape.reset()
    # checkpoint: parameters and buffers come back bit for bit
    d = Path(tempfile.mkdtemp())
    tr.save_checkpoint(d / "res.txt")
    assert "buffers 10" in (d / "res.txt").read_text().splitlines()
    saved = _state(model)
    for t in model.parameters() + model.buffers():
        t.set_data(np.full(t.shape(), 7.0, F))
    tr.load_checkpoint(d / "res.txt")
    for a, b in zip(saved[0] + saved[1], model.parameters() + model.buffers()):
        assert np.array_equal(_bits(a), _bits(b.data()))
    # data parallel: per-rank statistics would let the replicas drift apart
    comm = T.Communicator.loopback()
    with pytest.raises(T.TaperError, match="batch normalisation is not supported"):
        T.Trainer(model, opt, sample_shape=(1, 28, 28), comm=comm)
    # quantize: the reference's message, before anything is allocated
    calib = T.Tensor(np.random.default_rng(2).standard_normal((4, 1, 28, 28)).astype(F), (4, 1, 28, 28))
    used = _pool_in_use(T)
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        model.quantize("int8")
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        model.quantize_static(calib)
    with pytest.raises(T.TaperError, match="Quantization not implemented for this module type"):
        blk.quantize("int8")
    assert _pool_in_use(T) == used
    del comm, tr, opt, model, blk, loader
    gc.collect()
    T.Tape.reset()
