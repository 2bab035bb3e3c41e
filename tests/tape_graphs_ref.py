"""Graphs that are no chains -- tensors with several consumers, parameters used more than once, the same tensor on both sides of an op,
roots that are no lone loss -- written ONCE against the common face of tests/backends.py, plus a float64 reference to judge them.

The reference (`Np64Backend`) is a small reverse-mode tape in numpy float64 that restates the REFERENCE's semantics, not textbook autograd:
closures replay in reverse recording order, every closure up to the root's (tape.rs:106-127); a gradient slot is None or accumulated into;
a max-pool's backward zeroes its planes first, so it overwrites what the slot held (Q5); in faithful mode a convolution is cut behind its
product, so only its bias receives a gradient (Q2), in full mode it is differentiable; ReLU masks on x > 0; a root whose node is number 0
is taken for "no node" while the zero sentinel is on (Q1).  Its forward also notes how far every ReLU pre-activation lies from 0 and how
far apart the two largest values of every pool window lie, relative to the tensor's scale (`Tape.margins`): the inputs below are chosen
so that an fp32 rounding cannot flip either decision, and tests/test_tape_graphs_oracle.py asserts it.

A graph is a function build(F, d) -> (root, leaves): F one of the three faces ("np64", "oracle", "hip"), d a dict of float32 arrays,
leaves a dict name -> tensor whose gradients the tests compare.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

MARGIN = 1e-3   # every ReLU pre-activation / pool-window gap is at least this far from a tie, in units of its tensor's scale


# ================================================================ the float64 tape
class _TapeState:
    nodes: list = []
    sentinel = True
    margins: list = []   # (kind, margin / scale) per ReLU and per max-pool of the forward passes since the last reset


class Np64Tape:
    @staticmethod
    def reset():
        _TapeState.nodes = []
        _TapeState.margins = []

    @staticmethod
    def len():
        return len(_TapeState.nodes)

    @staticmethod
    def set_zero_sentinel(on):
        _TapeState.sentinel = bool(on)

    @staticmethod
    def margins():
        return list(_TapeState.margins)


def _push(out, inputs, fn):
    """tape.rs:51-101: recorded only if an input requires a gradient; the node's id is the tape's length before the push"""
    if not any(t is not None and t.req for t in inputs):
        return
    out.req = True
    out.node = len(_TapeState.nodes)
    _TapeState.nodes.append((out, fn))


def _acc(t, v):
    """ops.rs:124-137: the slot is None (then zeros) or accumulated into"""
    v = np.asarray(v, np.float64).reshape(t.d.shape)
    t.g = v.copy() if t.g is None else t.g + v


class NTensor:
    def __init__(self, data=None, shape=None, _d=None):
        if _d is None:
            a = np.asarray(data, dtype=np.float32)   # the faces take float32 data; the arithmetic behind it is float64
            if shape is None:
                shape = a.shape if a.ndim else (1,)
            _d = a.astype(np.float64).reshape(tuple(int(s) for s in shape))
        self.d, self.g, self.req, self.node = _d, None, False, 0

    @staticmethod
    def scalar(v):
        return NTensor([v], (1,))

    def requires_grad(self):
        self.req = True
        return self

    def shape(self): return tuple(self.d.shape)
    def numel(self): return int(self.d.size)
    def data(self): return self.d.copy()
    def grad(self): return None if self.g is None else self.g.copy()
    grad_ref = grad
    def tape_node(self): return self.node
    def zero_grad(self): self.g = None

    def set_grad(self, g):
        self.g = None if g is None else np.asarray(g, np.float32).astype(np.float64).reshape(self.d.shape)

    def backward(self):   # tensor.rs:520-529
        self.g = np.ones_like(self.d)
        if self.node == 0 and _TapeState.sentinel:   # Q1
            return
        nodes = _TapeState.nodes
        if not nodes:
            return
        for i in range(min(self.node, len(nodes) - 1), -1, -1):
            out, fn = nodes[i]
            if out.g is not None:
                fn(out.g)

    # ---- element-wise (ops.rs): only the element COUNT has to match (Q12)
    def _ew(self, o, f):
        assert self.d.size == o.d.size, "Tensor dimensions must match"
        return NTensor(_d=f(self.d, o.d.reshape(self.d.shape)))

    def __add__(self, o):
        out = self._ew(o, np.add)
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g)), (b.req and _acc(b, g))))
        return out

    def __sub__(self, o):
        out = self._ew(o, np.subtract)
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g)), (b.req and _acc(b, -g))))
        return out

    def __mul__(self, o):
        out = self._ew(o, np.multiply)
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g.reshape(-1) * b.d.reshape(-1))), (b.req and _acc(b, g.reshape(-1) * a.d.reshape(-1)))))
        return out

    def __truediv__(self, o):
        out = self._ew(o, np.divide)
        a, b = self, o

        def bwd(g):
            g, ad, bd = g.reshape(-1), a.d.reshape(-1), b.d.reshape(-1)
            if a.req:
                _acc(a, g / bd)
            if b.req:
                _acc(b, -(g * ad / (bd * bd)))
        _push(out, (a, b), bwd)
        return out

    def matmul(self, o):
        assert self.d.ndim == 2 and o.d.ndim == 2 and self.d.shape[1] == o.d.shape[0]
        out = NTensor(_d=self.d @ o.d)
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g @ b.d.T)), (b.req and _acc(b, a.d.T @ g))))
        return out

    def linear(self, weight, bias=None, relu=False):
        """taper_amd's fused node (no counterpart in the reference): x W^T + b [+ ReLU] as ONE node, so the product, the transposed weight
        and the pre-activation have no gradient slots of their own -- which shows where backward() runs twice without a reset: the
        primitive spelling's intermediates keep what they received and hand it on again, a fused node has nothing to keep"""
        x, w, b = self, weight, bias
        pre = x.d @ w.d.T + (b.d[None, :] if b is not None else 0.0)
        if relu:
            _TapeState.margins.append(("relu", float(np.abs(pre).min() / max(np.abs(pre).max(), 1e-300))))
        out = NTensor(_d=np.where(pre > 0, pre, 0.0) if relu else pre)

        def bwd(g):
            g = np.where(pre > 0, g, 0.0) if relu else g
            if x.req:
                _acc(x, g @ w.d)
            if w.req:
                _acc(w, g.T @ x.d)
            if b is not None and b.req:
                _acc(b, g.sum(axis=0))
        _push(out, (x, w, b), bwd)
        return out

    def _unary(self, value, dfn):
        out = NTensor(_d=value)
        x = self
        _push(out, (x,), lambda g: _acc(x, dfn(g)))
        return out

    def relu(self):   # ops.rs:312-374: the mask is on the INPUT (Q15)
        x = self.d
        _TapeState.margins.append(("relu", float(np.abs(x).min() / max(np.abs(x).max(), 1e-300))))
        return self._unary(np.where(x > 0, x, 0.0), lambda g: np.where(x > 0, g, 0.0))

    def sigmoid(self):
        y = 1.0 / (1.0 + np.exp(-self.d))
        return self._unary(y, lambda g: g * y * (1.0 - y))

    def exp(self):
        y = np.exp(self.d)
        return self._unary(y, lambda g: g * y)

    def log(self):
        x = self.d
        return self._unary(np.log(x), lambda g: g / x)

    def pow(self, e):
        x, e = self.d, float(np.float32(e))
        return self._unary(np.power(x, e), lambda g: g * e * np.power(x, e - 1.0))

    def sqrt(self): return self.pow(0.5)

    def transpose(self):
        assert self.d.ndim == 2
        return self._unary(self.d.T.copy(), lambda g: g.T)

    def mean(self):
        n = self.d.size
        sh = self.d.shape
        return self._unary(np.array([self.d.sum() / n]), lambda g: np.full(sh, g.reshape(-1)[0] / n))

    def reshape(self, shape):   # a data copy with a node of its own (tensor.rs:803-840)
        sh = self.d.shape
        return self._unary(self.d.reshape(tuple(int(s) for s in shape)).copy(), lambda g: g.reshape(sh))
    view = reshape

    def flatten(self, start_dim):
        s = self.d.shape
        return self.reshape(s[:start_dim] + (int(np.prod(s[start_dim:])),))

    def squeeze(self, dim=None):
        s = self.d.shape
        if dim is None:
            new = tuple(v for v in s if v != 1)
        else:
            assert s[dim] == 1
            new = s[:dim] + s[dim + 1:]
        return self.reshape(new or (1,))

    def unsqueeze(self, dim):
        s = self.d.shape
        return self.reshape(s[:dim] + (1,) + s[dim:])

    def sum(self, dim=None, keepdim=False):
        sh = self.d.shape
        if dim is None:
            return self._unary(np.array([self.d.sum()]), lambda g: np.full(sh, g.reshape(-1)[0]))
        kept = self.d.sum(axis=dim, keepdims=True)
        val = kept if keepdim else kept.reshape([v for i, v in enumerate(sh) if i != dim] or [1])
        return self._unary(val.copy(), lambda g: np.broadcast_to(g.reshape(kept.shape), sh))

    def max(self, dim=None):   # no tape node (tensor.rs:1021-1083)
        if dim is None:
            return NTensor(_d=np.array([self.d.max()])), NTensor(_d=np.array([float(self.d.argmax())]))
        return NTensor(_d=self.d.max(axis=dim, keepdims=True)), NTensor(_d=self.d.argmax(axis=dim).astype(np.float64))

    def add_broadcast(self, o):
        if self.d.shape == o.d.shape:
            return self + o
        assert self.d.ndim == 2 and o.d.ndim == 1 and self.d.shape[1] == o.d.shape[0]
        out = NTensor(_d=self.d + o.d[None, :])
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g)), (b.req and _acc(b, g.sum(axis=0)))))
        return out

    def sub_broadcast_rows(self, o):
        if self.d.shape == o.d.shape:
            return self - o
        assert self.d.ndim == 2 and o.d.shape == (self.d.shape[0], 1)
        out = NTensor(_d=self.d - o.d)
        a, b = self, o
        _push(out, (a, b), lambda g: ((a.req and _acc(a, g)), (b.req and _acc(b, -g.sum(axis=1, keepdims=True)))))
        return out

    # ---- convolution as the reference spells it (tensor.rs:1221-1285): im2col, a product with the weight buffer REINTERPRETED as
    # [c_in * 9, c_out] (Q3), NHWC -> NCHW, the bias.  mode 0 (faithful): im2col and the NHWC -> NCHW copy return fresh tensors without
    # a node, so the chain is cut and only the bias is reached (Q2); mode 1: every link is differentiable
    def conv2d(self, weight, bias, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mode=0):
        n, c, h, w = self.d.shape
        co, ci, kh, kw = weight.d.shape
        assert (kh, kw) == (3, 3) and tuple(stride) == (1, 1) and tuple(dilation) == (1, 1) and ci == c and padding[0] == padding[1]
        p = int(padding[0])
        ho, wo = h + 2 * p - 2, w + 2 * p - 2
        xp = np.pad(self.d, ((0, 0), (0, 0), (p, p), (p, p)))
        col = np.empty((n, ho, wo, c, 3, 3))
        for kr in range(3):
            for kc in range(3):
                col[:, :, :, :, kr, kc] = xp[:, :, kr:kr + ho, kc:kc + wo].transpose(0, 2, 3, 1)
        col_t = NTensor(_d=col.reshape(n * ho * wo, c * 9))
        x = self

        def col2im(g):
            g = g.reshape(n, ho, wo, c, 3, 3)
            gp = np.zeros_like(xp)
            for kr in range(3):
                for kc in range(3):
                    gp[:, :, kr:kr + ho, kc:kc + wo] += g[:, :, :, :, kr, kc].transpose(0, 3, 1, 2)
            _acc(x, gp[:, :, p:p + h, p:p + w])
        if mode == 1:
            _push(col_t, (x,), col2im)
        w2 = weight.reshape((c * 9, co))
        o4 = col_t.matmul(w2).reshape((n, ho, wo, co))
        nchw = NTensor(_d=o4.d.transpose(0, 3, 1, 2).copy())
        if mode == 1:
            _push(nchw, (o4,), lambda g: _acc(o4, g.transpose(0, 2, 3, 1)))
        if bias is None:
            return nchw
        out = NTensor(_d=nchw.d + bias.d[None, :, None, None])
        _push(out, (nchw, bias), lambda g: ((nchw.req and _acc(nchw, g)), (bias.req and _acc(bias, g.sum(axis=(0, 2, 3))))))
        return out

    def conv2d_relu(self, weight, bias, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mode=0):
        return self.conv2d(weight, bias, stride, padding, dilation, mode).relu()

    def _windows(self, k, s, p):
        n, c, h, w = self.d.shape
        s = tuple(s) if s else tuple(k)
        ho, wo = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
        for oh in range(ho):
            for ow in range(wo):
                r0, r1 = max(oh * s[0] - p[0], 0), min(oh * s[0] - p[0] + k[0], h)
                c0, c1 = max(ow * s[1] - p[1], 0), min(ow * s[1] - p[1] + k[1], w)
                yield oh, ow, r0, r1, c0, c1
        return

    def max_pool2d(self, kernel_size, stride=None, padding=(0, 0)):   # tensor.rs:1391-1521
        n, c, h, w = self.d.shape
        s = tuple(stride) if stride else tuple(kernel_size)
        ho, wo = (h + 2 * padding[0] - kernel_size[0]) // s[0] + 1, (w + 2 * padding[1] - kernel_size[1]) // s[1] + 1
        out, arg = np.empty((n, c, ho, wo)), np.empty((n, c, ho, wo, 2), np.int64)
        gap = np.inf
        for oh, ow, r0, r1, c0, c1 in self._windows(kernel_size, stride, padding):
            win = self.d[:, :, r0:r1, c0:c1].reshape(n, c, -1)
            best = win.argmax(axis=2)   # the first maximum, like the reference's strict >
            out[:, :, oh, ow] = np.take_along_axis(win, best[..., None], 2)[..., 0]
            arg[:, :, oh, ow, 0], arg[:, :, oh, ow, 1] = r0 + best // (c1 - c0), c0 + best % (c1 - c0)
            if win.shape[2] > 1:
                top = np.sort(win, axis=2)
                gap = min(gap, float((top[..., -1] - top[..., -2]).min()))
        _TapeState.margins.append(("maxpool", gap / max(float(np.abs(self.d).max()), 1e-300)))
        res, x = NTensor(_d=out), self

        def bwd(g):   # the planes are zeroed first: whatever the slot held is overwritten (Q5)
            gi = np.zeros_like(x.d)
            ni, ci = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
            for oh in range(ho):
                for ow in range(wo):
                    np.add.at(gi, (ni, ci, arg[:, :, oh, ow, 0], arg[:, :, oh, ow, 1]), g[:, :, oh, ow])
            x.g = gi
        _push(res, (x,), bwd)
        return res

    def avg_pool2d(self, kernel_size, stride=None, padding=(0, 0)):   # tensor.rs:1524-1660: the padding counts in the divisor (Q6)
        n, c, h, w = self.d.shape
        s = tuple(stride) if stride else tuple(kernel_size)
        ho, wo = (h + 2 * padding[0] - kernel_size[0]) // s[0] + 1, (w + 2 * padding[1] - kernel_size[1]) // s[1] + 1
        div = float(kernel_size[0] * kernel_size[1])
        out = np.empty((n, c, ho, wo))
        wins = list(self._windows(kernel_size, stride, padding))
        for oh, ow, r0, r1, c0, c1 in wins:
            out[:, :, oh, ow] = self.d[:, :, r0:r1, c0:c1].sum(axis=(2, 3)) / div
        res, x = NTensor(_d=out), self

        def bwd(g):
            gi = np.zeros_like(x.d)
            for oh, ow, r0, r1, c0, c1 in wins:
                gi[:, :, r0:r1, c0:c1] += (g[:, :, oh, ow] / div)[:, :, None, None]
            _acc(x, gi)
        _push(res, (x,), bwd)
        return res


def _np_log_softmax(x):   # loss.rs:101-126: a chain of recorded primitives; the row maximum is a constant (max has no node)
    shifted = x.sub_broadcast_rows(x.max(1)[0])
    return shifted.sub_broadcast_rows(shifted.exp().sum(1, True).log())


def _np_cross_entropy(logits, targets):   # loss.rs:136-195: ONE node on the logits; (softmax - onehot) * gout / B
    b, c = logits.d.shape
    logp = _np_log_softmax(logits)
    cls = targets.d.reshape(-1).astype(np.int64)
    out = NTensor(_d=np.array([-logp.d[np.arange(b), cls].sum() / b]))

    def bwd(g):
        if logp.req:   # the reference forms the softmax with a recorded exp DURING backward (Q7): the tape grows by a node
            _TapeState.nodes.append((NTensor(_d=np.zeros(1)), lambda _g: None))
        sm = np.exp(logp.d)
        sm[np.arange(b), cls] -= 1.0
        _acc(logits, sm * (g.reshape(-1)[0] / b))
    _push(out, (logits,), bwd)
    return out


def _np_cross_entropy_onehot(logits, targets):   # loss.rs:201-245: (softmax - t) * gout / B whatever the rows of t sum to
    b = logits.d.shape[0]
    sh = logits.d - logits.d.max(axis=1, keepdims=True)
    logp = sh - np.log(np.exp(sh).sum(axis=1, keepdims=True))
    out = NTensor(_d=np.array([-(targets.d * logp).sum() / b]))
    _push(out, (logits,), lambda g: _acc(logits, (np.exp(logp) - targets.d) * (g.reshape(-1)[0] / b)))
    return out


def _np_bce(pred, targets):   # loss.rs:6-73
    n = pred.d.size
    p, y = np.clip(pred.d, float(np.float32(1e-7)), 1.0 - float(np.float32(1e-7))), targets.d.reshape(pred.d.shape)
    out = NTensor(_d=np.array([-(y * np.log(p) + (1 - y) * np.log(1 - p)).sum() / n]))

    def bwd(g):
        g0 = g.reshape(-1)[0]
        if pred.req:
            _acc(pred, g0 * (-(y / p - (1 - y) / (1 - p))) / n)
        if targets.req:
            _acc(targets, g0 * (np.log(1 - p) - np.log(p)) / n)
    _push(out, (pred, targets), bwd)
    return out


def _np_mse(pred, targets):   # loss.rs:76-80
    d = pred - targets
    return (d * d).mean()


def _np_one_hot(idx, num_classes):
    return NTensor(_d=np.eye(num_classes)[idx.d.reshape(-1).astype(np.int64)])


class Np64Backend:
    name = "np64"
    Tensor, Tape = NTensor, Np64Tape
    cross_entropy_loss = staticmethod(_np_cross_entropy)
    log_softmax = staticmethod(lambda x, dim=-1: _np_log_softmax(x))
    softmax = staticmethod(lambda x, dim=-1: _np_log_softmax(x).exp())
    mse_loss, bce_loss, one_hot = staticmethod(_np_mse), staticmethod(_np_bce), staticmethod(_np_one_hot)
    cross_entropy_loss_onehot = staticmethod(_np_cross_entropy_onehot)

    def set_zero_sentinel(self, on):
        Np64Tape.set_zero_sentinel(on)


def face(name):
    """one of the three faces, with the few calls tests/backends.py leaves to the modules underneath"""
    if name == "np64":
        return Np64Backend()
    from tests import backends
    F = backends.get(name)
    F.bce_loss = F.m.bce_loss
    F.cross_entropy_loss_onehot = getattr(F.m, "cross_entropy_loss_onehot", None)   # (the oracle records no such node: hip and np64 only)
    return F


def reset(F, sentinel=None):
    """an empty tape, faithful mode; the zero sentinel as asked (default: each face's own default is left alone)"""
    F.Tape.reset()
    if F.name == "hip":
        F.m.set_full_backward(False)
    if sentinel is not None:
        F.set_zero_sentinel(sentinel)


# ================================================================ spellings the faces differ in
def leaf(F, a, grad=True):
    t = F.Tensor(np.asarray(a, np.float32))
    return t.requires_grad() if grad else t


def lin(F, x, w, b, relu=False, fused=False):
    """a Linear (nn.rs:54-60) as the reference records it, or as the one fused node every taper_amd Linear module records"""
    if fused:
        assert F.name in ("hip", "np64"), "Tensor.linear: taper_amd's node, restated on the float64 tape; the oracle has none"
        return x.linear(w, b, relu)
    y = x.matmul(w.transpose()).add_broadcast(b)
    return y.relu() if relu else y


def conv_relu(F, x, w, b, full):
    """Conv2dReLU 3x3, stride 1, padding 1 in faithful (Q2) or full-backward mode"""
    if F.name == "hip":
        F.m.set_full_backward(bool(full))
        return x.conv2d_relu(w, b, (1, 1), (1, 1))
    return x.conv2d_relu(w, b, (1, 1), (1, 1), (1, 1), mode=1 if full else 0)


def wsum(F, t, w):
    """(w . t).sum() with a constant w of t's shape: a scalar whose gradient on t is w"""
    return (t * F.Tensor(np.asarray(w, np.float32))).sum()


def grads(leaves):
    return {k: t.grad() for k, t in leaves.items()}


# ================================================================ inputs
def _signed(rng, shape, lo, hi):
    return (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def data_graph1(seed=3):
    """x[5,7] -> relu(7 -> 6) -> {tied 6 -> 6 twice, head 6 -> 4}.  (seed: the first for which every ReLU clears MARGIN in float64)"""
    rng = np.random.default_rng(seed)
    return dict(x=rng.standard_normal((5, 7)).astype(np.float32), W1=rng.uniform(-0.6, 0.6, (6, 7)).astype(np.float32),
                b1=rng.uniform(-0.2, 0.2, 6).astype(np.float32), W2=rng.uniform(-0.7, 0.7, (6, 6)).astype(np.float32),
                b2=rng.uniform(-0.2, 0.2, 6).astype(np.float32), W3=rng.uniform(-0.7, 0.7, (4, 6)).astype(np.float32),
                b3=rng.uniform(-0.2, 0.2, 4).astype(np.float32), y=rng.integers(0, 4, 5).astype(np.float32))


def data_graph2(batch=512, inf=16, hidden=2048, classes=10, seed=2):
    """h[batch, hidden] of about a million elements cannot clear MARGIN by the luck of a seed: the sign of every pre-activation is
    built in -- |x| and |W1| in [0.5, 1], row r of x carries the sign s_r and row c of W1 the sign t_c, so x W1^T has the sign s_r t_c
    and a magnitude of at least inf / 4, and the bias stays below 0.1.  Half of h's mask is on, in a pattern of both indices."""
    rng = np.random.default_rng(seed)
    s, t = rng.choice([-1.0, 1.0], (batch, 1)), rng.choice([-1.0, 1.0], (hidden, 1))
    return dict(x=(rng.uniform(0.5, 1.0, (batch, inf)) * s).astype(np.float32), W1=(rng.uniform(0.5, 1.0, (hidden, inf)) * t / inf).astype(np.float32),
                b1=rng.uniform(-0.1, 0.1, hidden).astype(np.float32) / np.float32(inf),
                Wa=rng.uniform(-0.05, 0.05, (classes, hidden)).astype(np.float32), ba=rng.uniform(-0.1, 0.1, classes).astype(np.float32),
                Wb=rng.uniform(-0.05, 0.05, (classes, hidden)).astype(np.float32), bb=rng.uniform(-0.1, 0.1, classes).astype(np.float32),
                y=rng.integers(0, classes, batch).astype(np.float32))


def _spread(rng, shape, lo, hi):
    """distinct values, evenly spaced over +-[lo, hi] and shuffled: no two closer than the spacing, none closer to 0 than lo"""
    n = int(np.prod(shape))
    v = np.linspace(lo, hi, n) * rng.choice([-1.0, 1.0], n)
    return rng.permutation(v).reshape(shape).astype(np.float32)


def data_graph3(c_in=2, c_out=3, seed=5):
    rng = np.random.default_rng(seed)
    bound = np.sqrt(6.0 / (c_in * 9))
    return dict(x=rng.standard_normal((2, c_in, 4, 4)).astype(np.float32), w=rng.uniform(-bound, bound, (c_out, c_in, 3, 3)).astype(np.float32),
                b=rng.uniform(0.1, 0.3, c_out).astype(np.float32), wp=rng.uniform(0.5, 1.5, (2, c_out, 2, 2)).astype(np.float32),
                wg=rng.uniform(0.5, 1.5, (2, c_out, 1, 1)).astype(np.float32), wq=rng.uniform(0.5, 1.5, (2, c_out, 4, 4)).astype(np.float32))


# ================================================================ graph 1: shared hidden tensor, tied weights
def graph1(order, fused=False):
    def build(F, d):
        L = {k: leaf(F, d[k]) for k in ("x", "W1", "b1", "W2", "b2", "W3", "b3")}
        y = F.Tensor(d["y"])
        h = lin(F, L["x"], L["W1"], L["b1"], True, fused)
        tied = lambda: lin(F, lin(F, h, L["W2"], L["b2"], True, fused), L["W2"], L["b2"], True, fused)   # noqa: E731
        if order == 0:      # the tied branch is h's first consumer
            t = tied()
            ot, oh = lin(F, t, L["W3"], L["b3"], False, fused), lin(F, h, L["W3"], L["b3"], False, fused)
        else:               # the head is
            oh = lin(F, h, L["W3"], L["b3"], False, fused)
            ot = lin(F, tied(), L["W3"], L["b3"], False, fused)
        return F.cross_entropy_loss(ot + oh, y), L
    return build


# ================================================================ graph 2: the dX epilogue hands over a masked gradient
def graph2(variant, order=0, fused=False):
    """variant "two": two heads on h; "square": one head and h * h; "one": the single-consumer control"""
    def build(F, d):
        names = ("x", "W1", "b1", "Wa", "ba") + (("Wb", "bb") if variant == "two" else ())
        L = {k: leaf(F, d[k]) for k in names}
        y = F.Tensor(d["y"])
        h = lin(F, L["x"], L["W1"], L["b1"], True, fused)
        head_a = lambda: lin(F, h, L["Wa"], L["ba"], False, fused)   # noqa: E731
        if variant == "one":
            return F.cross_entropy_loss(head_a(), y), L
        if variant == "two":
            head_b = lambda: lin(F, h, L["Wb"], L["bb"], False, fused)   # noqa: E731
            a, b = (head_a(), head_b()) if order == 0 else tuple(reversed((head_b(), head_a())))
            return F.cross_entropy_loss(a + b, y), L
        if order == 0:
            ce, sq = F.cross_entropy_loss(head_a(), y), (h * h).mean()
        else:
            sq = (h * h).mean()
            ce = F.cross_entropy_loss(head_a(), y)
        return ce + sq, L
    return build


# ================================================================ graph 3: a Conv2dReLU output with two consumers
def graph3(pool, order, full):
    """pool "max": MaxPool2d(2) (Q5: it overwrites); "avg": the global average pool.  order 0: the pool is recorded first (so it replays
    LAST, over a slot a * a already wrote); order 1: a * a first"""
    def build(F, d):
        L = dict(x=leaf(F, d["x"]), w=leaf(F, d["w"]), b=leaf(F, d["b"]))
        a = conv_relu(F, L["x"], L["w"], L["b"], full)
        pooled = (lambda: wsum(F, a.max_pool2d((2, 2)), d["wp"])) if pool == "max" else (lambda: wsum(F, a.avg_pool2d((4, 4)), d["wg"]))
        square = lambda: wsum(F, a * a, d["wq"])   # noqa: E731
        if order == 0:
            p, q = pooled(), square()
        else:
            q, p = square(), pooled()
        return p + q, L
    return build


def graph3_tied(full=True):
    """c_in = 8, c_out = 16 (the matrix-core gradient kernels), the SAME convolution applied to x twice: the second node to replay finds
    the slots of x, w and b held and accumulates.  (No max-pool here: among 128 windows of a ReLU output some are all zeros, a tie.)"""
    def build(F, d):
        L = dict(x=leaf(F, d["x"]), w=leaf(F, d["w"]), b=leaf(F, d["b"]))
        a1 = conv_relu(F, L["x"], L["w"], L["b"], full)
        a2 = conv_relu(F, L["x"], L["w"], L["b"], full)
        return wsum(F, a1.avg_pool2d((4, 4)), d["wg"]) + wsum(F, a2 * a2, d["wq"]), L
    return build


# ================================================================ graph 4: the same tensor on both sides
def data_graph4(n=1027, seed=4):
    rng = np.random.default_rng(seed)
    return dict(x=_signed(rng, n, 0.5, 2.0), w=rng.uniform(-1, 1, n).astype(np.float32), m=_signed(rng, (9, 9), 0.2, 1.0),
                wm=rng.uniform(-1, 1, (9, 9)).astype(np.float32))


def graph4(op):
    def build(F, d):
        if op == "matmul":
            x = leaf(F, d["m"])
            return wsum(F, x.matmul(x), d["wm"]), dict(x=x)
        if op == "add_broadcast":
            x = leaf(F, d["m"])
            return wsum(F, x.add_broadcast(x), d["wm"]), dict(x=x)
        x = leaf(F, d["x"])
        if op == "div_view":     # b: a reshape of a -- the same values (on hip the same storage), a gradient slot of its own
            r = x / x.reshape((d["x"].size,))
        else:
            r = dict(add=lambda: x + x, sub=lambda: x - x, mul=lambda: x * x, div=lambda: x / x)[op]()
        return wsum(F, r, d["w"]), dict(x=x)
    return build


GRAPH4_OPS = ("add", "sub", "mul", "div", "matmul", "add_broadcast", "div_view")


# ================================================================ graph 5: every differentiable op on an empty and on a held slot
def _pos(rng, shape): return rng.uniform(0.5, 2.0, shape).astype(np.float32)


def _ops_table():
    """name -> (input maker(rng) -> dict, op(F, x, d) -> tensor).  d["x"] is the leaf; everything else in d is a constant"""
    T = {}
    two = lambda rng: dict(x=_signed(rng, (6, 10), 0.2, 1.0))   # noqa: E731
    pos = lambda rng: dict(x=_pos(rng, (6, 10)))   # noqa: E731
    T["relu"] = (two, lambda F, x, d: x.relu())
    T["sigmoid"] = (two, lambda F, x, d: x.sigmoid())
    T["exp"] = (two, lambda F, x, d: x.exp())
    T["log"] = (pos, lambda F, x, d: x.log())
    T["pow0.5"] = (pos, lambda F, x, d: x.pow(0.5))
    T["pow3"] = (two, lambda F, x, d: x.pow(3.0))
    T["transpose"] = (two, lambda F, x, d: x.transpose())
    T["reshape"] = (two, lambda F, x, d: x.reshape((10, 6)))
    T["flatten"] = (lambda rng: dict(x=_signed(rng, (2, 3, 4, 4), 0.2, 1.0)), lambda F, x, d: x.flatten(1))
    T["squeeze"] = (lambda rng: dict(x=_signed(rng, (6, 1, 10), 0.2, 1.0)), lambda F, x, d: x.squeeze(1))
    T["unsqueeze"] = (two, lambda F, x, d: x.unsqueeze(1))
    three = lambda rng: dict(x=_signed(rng, (4, 5, 6), 0.2, 1.0))   # noqa: E731
    for dim, nm in ((0, "first"), (2, "last"), (1, "middle")):
        for keep in (False, True):
            T[f"sum_{nm}{'_keepdim' if keep else ''}"] = (three, lambda F, x, d, dim=dim, keep=keep: x.sum(dim, keep))
    T["sum_rows_2d"] = (two, lambda F, x, d: x.sum(1, True))
    T["sum_all"] = (two, lambda F, x, d: x.sum())
    T["mean"] = (two, lambda F, x, d: x.mean())
    T["add_broadcast_lhs"] = (lambda rng: dict(x=_signed(rng, (6, 10), 0.2, 1.0), c=_signed(rng, 10, 0.2, 1.0)),
                              lambda F, x, d: x.add_broadcast(F.Tensor(d["c"])))
    T["add_broadcast_rhs"] = (lambda rng: dict(x=_signed(rng, 10, 0.2, 1.0), c=_signed(rng, (6, 10), 0.2, 1.0)),
                              lambda F, x, d: F.Tensor(d["c"]).add_broadcast(x))
    T["sub_broadcast_rows_lhs"] = (lambda rng: dict(x=_signed(rng, (6, 10), 0.2, 1.0), c=_signed(rng, (6, 1), 0.2, 1.0)),
                                   lambda F, x, d: x.sub_broadcast_rows(F.Tensor(d["c"])))
    T["sub_broadcast_rows_rhs"] = (lambda rng: dict(x=_signed(rng, (6, 1), 0.2, 1.0), c=_signed(rng, (6, 10), 0.2, 1.0)),
                                   lambda F, x, d: F.Tensor(d["c"]).sub_broadcast_rows(x))
    img = lambda rng: dict(x=_spread(rng, (2, 3, 4, 4), 0.2, 1.0))   # noqa: E731
    T["max_pool2d"] = (img, lambda F, x, d: x.max_pool2d((2, 2)))
    T["max_pool2d_3x3_pad"] = (img, lambda F, x, d: x.max_pool2d((3, 3), (2, 2), (1, 1)))
    T["max_pool2d_global"] = (img, lambda F, x, d: x.max_pool2d((4, 4)))
    T["avg_pool2d"] = (img, lambda F, x, d: x.avg_pool2d((2, 2)))
    T["avg_pool2d_3x3_pad"] = (img, lambda F, x, d: x.avg_pool2d((3, 3), (2, 2), (1, 1)))
    T["avg_pool2d_global"] = (img, lambda F, x, d: x.avg_pool2d((4, 4)))
    T["log_softmax"] = (two, lambda F, x, d: F.log_softmax(x))
    T["softmax"] = (two, lambda F, x, d: F.softmax(x))
    cls = lambda rng: dict(x=_signed(rng, (6, 10), 0.2, 1.0), y=rng.integers(0, 10, 6).astype(np.float32))   # noqa: E731
    T["cross_entropy_loss"] = (cls, lambda F, x, d: F.cross_entropy_loss(x, F.Tensor(d["y"])))
    T["cross_entropy_loss_onehot"] = (cls, lambda F, x, d: F.cross_entropy_loss_onehot(x, F.one_hot(F.Tensor(d["y"]), 10)))
    T["mse_loss"] = (lambda rng: dict(x=_signed(rng, (6, 10), 0.2, 1.0), t=_signed(rng, (6, 10), 0.2, 1.0)),
                     lambda F, x, d: F.mse_loss(x, F.Tensor(d["t"])))
    T["bce_loss"] = (lambda rng: dict(x=rng.uniform(0.1, 0.9, (6, 10)).astype(np.float32), t=rng.integers(0, 2, (6, 10)).astype(np.float32)),
                     lambda F, x, d: F.bce_loss(x, F.Tensor(d["t"])))
    return T


OPS = _ops_table()
RESHAPE_FAMILY = ("reshape", "flatten", "squeeze", "unsqueeze")
Q5_OPS = ("max_pool2d", "max_pool2d_3x3_pad", "max_pool2d_global")   # order 0 overwrites exp's term: the two orders must differ
ORACLE_LACKS = ("cross_entropy_loss_onehot",)                        # the oracle's Python face records no such node


def data_graph5(name):
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    d = OPS[name][0](rng)
    d["_name"] = name
    return d


def graph5(name, order, solo=False):
    """(w . op(x)).sum() + (w' . exp(x)).sum().  order 0: op is recorded first, so its backward finds the slot HELD by exp's;
    order 1: op last, its backward finds the slot empty.  solo: the op's term alone (its gradient into an empty slot and nothing else)"""
    def build(F, d):
        import zlib
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
        x = leaf(F, d["x"])
        op = OPS[name][1]
        wide = lambda: wsum(F, x.exp(), w2)   # noqa: E731
        w2 = rng.uniform(0.5, 1.5, d["x"].shape).astype(np.float32)
        if order == 0:
            r = op(F, x, d)
            w1 = rng.uniform(0.5, 1.5, r.shape()).astype(np.float32)
            a = wsum(F, r, w1)
            return (a if solo else a + wide()), dict(x=x)
        e = wide()
        r = op(F, x, d)
        w1 = rng.uniform(0.5, 1.5, r.shape()).astype(np.float32)
        return wsum(F, r, w1) + e, dict(x=x)
    return build


def graph5_solo_weight(name, x_shape, out_shape):
    """the w of graph5(name, 0, solo=True): the second draw of the graph's generator"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    rng.uniform(0.5, 1.5, x_shape)
    return rng.uniform(0.5, 1.5, out_shape).astype(np.float32)


# ================================================================ graph 6: roots and repetition
def data_graph6(seed=6):
    rng = np.random.default_rng(seed)
    return dict(k=rng.uniform(-1, 1, 3).astype(np.float32), z=rng.standard_normal((5, 4)).astype(np.float32), y=rng.integers(0, 4, 5).astype(np.float32),
                x=rng.standard_normal((5, 7)).astype(np.float32), W=rng.uniform(-0.6, 0.6, (4, 7)).astype(np.float32),
                b=rng.uniform(-0.2, 0.2, 4).astype(np.float32), z2=rng.standard_normal((5, 4)).astype(np.float32),
                t2=rng.standard_normal((5, 4)).astype(np.float32), w=rng.uniform(0.5, 1.5, (5, 4)).astype(np.float32),
                seed=rng.standard_normal((5, 4)).astype(np.float32))


def _node0(F, d):
    """an unrelated first node: no root below is node 0 in any spelling, so the zero sentinel (Q1) changes nothing where it is not the subject"""
    return leaf(F, d["k"]).exp()


def graph6(kind, fused=False):
    def build(F, d):
        keep = _node0(F, d)
        if kind == "leaf_logits":       # cross-entropy on a LEAF: the root's upstream gradient is the constant 1, the slot None
            z = leaf(F, d["z"])
            root, L = F.cross_entropy_loss(z, F.Tensor(d["y"])), dict(z=z)
        elif kind == "linear_logits":   # ... behind a Linear: the logits are an intermediate whose gradient zero_grad never clears
            L = dict(x=leaf(F, d["x"]), W=leaf(F, d["W"]), b=leaf(F, d["b"]))
            root = F.cross_entropy_loss(lin(F, L["x"], L["W"], L["b"], False, fused), F.Tensor(d["y"]))
        elif kind == "nonscalar_root":
            z = leaf(F, d["z"])
            root, L = z * F.Tensor(d["w"]), dict(z=z)
        elif kind == "seeded":          # the slot already holds what set_grad put there
            z = leaf(F, d["z"])
            z.set_grad(d["seed"])
            root, L = F.cross_entropy_loss(z, F.Tensor(d["y"])), dict(z=z)
        elif kind == "loss_times_loss":  # a cross-entropy that is an INPUT of the root: its upstream gradient is no constant 1
            z, z2 = leaf(F, d["z"]), leaf(F, d["z2"])
            root, L = F.cross_entropy_loss(z, F.Tensor(d["y"])) * F.mse_loss(z2, F.Tensor(d["t2"])), dict(z=z, z2=z2)
        elif kind == "one_operand_constant":
            z, c = leaf(F, d["z"]), leaf(F, d["z2"], grad=False)
            root, L = wsum(F, z * c, d["w"]) + wsum(F, z / c, d["w"]), dict(z=z, c=c)
        else:
            raise ValueError(kind)
        L["_keep"] = keep
        return root, L
    return build


GRAPH6_KINDS = ("leaf_logits", "linear_logits", "nonscalar_root", "seeded", "loss_times_loss", "one_operand_constant")


def run_repeated(F, build, d, sentinel=None):
    """backward twice without zero_grad, then zero_grad on the leaves and a third backward: the leaves' gradients after each stage"""
    reset(F, sentinel)
    root, L = build(F, d)
    L = {k: t for k, t in L.items() if not k.startswith("_")}
    stages = []
    root.backward()
    stages.append(grads(L))
    root.backward()
    stages.append(grads(L))
    for t in L.values():
        t.zero_grad()
    root.backward()
    stages.append(grads(L))
    value = np.asarray(root.data(), np.float64)
    reset(F, None if sentinel is None else (F.name != "hip"))
    return value, stages


def graph_root_is_node0():
    """Q1 itself: the root is the tape's first node in every spelling.  Sentinel on: backward() stops at the root; off: x.grad = exp(x)"""
    def build(F, d):
        x = leaf(F, d["k"])
        return x.exp(), dict(x=x)
    return build


def run(F, build, d, sentinel=None):
    """one forward and one backward on an empty tape -> (root value, {leaf: gradient or None}, tape length after backward)"""
    reset(F, sentinel)
    root, L = build(F, d)
    L = {k: t for k, t in L.items() if not k.startswith("_")}
    root.backward()
    out = np.asarray(root.data(), np.float64), grads(L), F.Tape.len()
    margins = Np64Tape.margins() if F.name == "np64" else None
    reset(F, None if sentinel is None else (F.name != "hip"))   # (the faces' own defaults: on for the reference's two, off for taper_amd)
    return out + (margins,)


def err_over_scale(got, ref, scale=None):
    """max |got - ref| over the tensor's scale max |ref| -- or over `scale` where the reference is a cancellation down to 0 (x / x)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64).reshape(np.shape(got))
    scale = float(np.abs(ref).max()) if scale is None else float(scale)
    return float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())


def graph4_scale(op, d):
    """x / x: the gradient is g / x - g x / x^2 = 0, two terms of size |w / x| that cancel -- their size is the scale of an error there"""
    return float(np.abs(d["w"].astype(np.float64) / d["x"]).max()) if op in ("div", "div_view") else None


# ================================================================ graph 7: a Trainer step over a tied layer, as the oracle trains it
def data_graph7(seed=7, batch=8, steps=3):
    rng = np.random.default_rng(seed)
    u = lambda o, i: rng.uniform(-np.sqrt(2.0 / i), np.sqrt(2.0 / i), (o, i)).astype(np.float32)   # noqa: E731
    return dict(W0=u(32, 784), b0=rng.uniform(-0.1, 0.1, 32).astype(np.float32), WL=u(32, 32), bL=rng.uniform(-0.1, 0.1, 32).astype(np.float32),
                W3=u(10, 32), b3=rng.uniform(-0.1, 0.1, 10).astype(np.float32),
                xs=(rng.integers(0, 256, (steps, batch, 784)) / 255.0).astype(np.float32), ys=rng.integers(0, 10, (steps, batch)).astype(np.float32))


def oracle_tied_training(d, lr=1e-3):
    """Sequential[Linear(784,32), ReLU, L, ReLU, L, ReLU, Linear(32,10)] with ONE L, by hand on the oracle: primitive ops, one Adam over the
    six distinct parameters -> (losses, parameters, first moments, second moments)"""
    from oracle import oracle as O
    O.Tape.set_zero_sentinel(True)
    P = [O.Tensor(d[k]).requires_grad() for k in ("W0", "b0", "WL", "bL", "W3", "b3")]
    opt = O.Adam(P, lr)
    losses = []
    for x, y in zip(d["xs"], d["ys"]):
        O.Tape.reset()
        h = O.Tensor(x).matmul(P[0].transpose()).add_broadcast(P[1]).relu()
        for _ in range(2):
            h = h.matmul(P[2].transpose()).add_broadcast(P[3]).relu()
        loss = O.cross_entropy_loss(h.matmul(P[4].transpose()).add_broadcast(P[5]), O.Tensor(y))
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.data()[0]))
    O.Tape.reset()
    return losses, [p.data() for p in P], [opt.m(i) for i in range(6)], [opt.v(i) for i in range(6)]
