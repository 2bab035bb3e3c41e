"""Quantization-aware training on the GPU (src/quantization/{fake_quantize,qat_layers,qat_manager}.rs): the fake-quant kernels bit for bit
against the oracle's codecs and a numpy restatement of the symmetric activation formula, the straight-through estimator against the
oracle's gradients on the fake-quantized weights, whole QAT training runs (eager and captured, fused Adam on and off) against an oracle
loop, deployment through quantize(), the mode switches and the example driver."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from oracle import train_extra as OX
from tests import backends

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RTOL = 1e-4
f32 = np.float32


def _err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / max(1.0, float(np.abs(ref).max())))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def fq_int8(x):   # quantize() + dequantize of the storage codecs (tensor.rs:2110-2152, 353-360)
    q, scale, zp, mn = OX.quantize_int8(x)
    return OX.dequantize_int8(q, scale, zp, mn).reshape(np.shape(x)), (mn, scale)


def fq_f16(x):
    return OX.f16_bits_to_f32(OX.f32_to_f16_bits(np.asarray(x, f32))).reshape(np.shape(x))


def fq_act_int8(x):
    """fake_quantize.rs:71-118, 155-162, symmetric (zero point 0): finite min / max with the reference's edge cases, scale = max_abs / 127,
    y = clamp(round(x / scale) as i32, -128, 127) * scale"""
    x = np.asarray(x, f32)
    fin = x[np.isfinite(x)]
    mn, mx = (f32(fin.min()), f32(fin.max())) if fin.size else (f32(np.inf), f32(-np.inf))
    if mn == mx:
        mn, mx = (f32(0), f32(1)) if mn == 0 else (f32(mn * f32(0.9)), f32(mn * f32(1.1)))
    scale = f32(max(abs(mn), abs(mx)) / f32(127))
    with np.errstate(all="ignore"):
        t = (x / scale).astype(f32).astype(np.float64)
        r = np.sign(t) * np.floor(np.abs(t) + 0.5)                          # f32::round (exact in f64)
        r = np.clip(np.nan_to_num(r, nan=0.0, posinf=2147483647.0, neginf=-2147483648.0), -2147483648.0, 2147483647.0)
        q = np.clip(r.astype(np.int64), -128, 127)
        return (q.astype(f32) * scale).astype(f32), scale


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _fq_multi(ctx, arrays, qtypes):
    """th_fake_quant_multi over the list -> ([y], [params])"""
    from taper_amd import hip as H
    xs = [ctx.upload(a) for a in arrays]
    ys = [ctx.empty(max(a.size, 1)) for a in arrays]
    ps = [ctx.empty(2) for _ in arrays]
    for p in ps:
        ctx.call("th_fill_f32", p, float("nan"), 2)
    items = (H.FqItem * len(arrays))(*[H.FqItem(int(x), int(y), int(p), a.size, 0 if q == "int8" else 1)
                                       for x, y, p, a, q in zip(xs, ys, ps, arrays, qtypes)])
    d_items = ctx.upload(np.frombuffer(bytes(items), np.uint8))
    ctx.call("th_fake_quant_multi", d_items, len(arrays))
    return [ctx.download(y, a.shape) for y, a in zip(ys, arrays)], [ctx.download(p, (2,)) for p in ps]


def _edge_inputs(rng):
    a = rng.standard_normal(1000).astype(f32)
    a[[3, 500]] = [np.inf, -np.inf]
    b = rng.standard_normal(777).astype(f32)
    b[[0, 7, 776]] = np.nan
    return dict(inf=a, nan=b, equal=np.full(300, 0.37, f32), equal_neg=np.full(5, -2.5, f32), zero=np.zeros(64, f32),
                all_nonfinite=np.array([np.inf, np.nan, -np.inf], f32))


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("qtype", ["int8", "float16"])
@pytest.mark.parametrize("n", [1, 255, 256 * 1024 + 3, 4096 * 4096])
def test_weight_kernel_bit_exact(ctx, qtype, n):
    x = (np.random.default_rng(n).standard_normal(n) * 0.05).astype(f32)
    (y,), (p,) = _fq_multi(ctx, [x], [qtype])
    if qtype == "int8":
        ref, (mn, scale) = fq_int8(x)
        assert _bits(p).tolist() == _bits([mn, scale]).tolist()
    else:
        ref = fq_f16(x)
    np.testing.assert_array_equal(_bits(y), _bits(ref))


@pytest.mark.parametrize("qtype", ["int8", "float16"])
def test_weight_kernel_edge_inputs_and_many_tensors(ctx, qtype):
    rng = np.random.default_rng(5)
    arrays = list(_edge_inputs(rng).values()) + [rng.standard_normal(n).astype(f32) for n in (1, 17, 4096, 100003, 784 * 128, 10)]
    arrays[-2] = arrays[-2].reshape(128, 784)
    ys, ps = _fq_multi(ctx, arrays, [qtype] * len(arrays))
    for a, y, p in zip(arrays, ys, ps):
        ref = fq_int8(a)[0] if qtype == "int8" else fq_f16(a)
        np.testing.assert_array_equal(_bits(y), _bits(ref))
        if qtype == "int8":   # the pair th_quantize_int8 writes
            q, dp = ctx.empty(a.size), ctx.empty(2)
            ctx.call("th_quantize_int8", ctx.upload(a), q, a.size, dp)
            assert _bits(p).tolist() == _bits(ctx.download(dp, (2,))).tolist()


def test_weight_kernel_mixed_list(ctx):
    rng = np.random.default_rng(6)
    arrays = [rng.standard_normal(n).astype(f32) for n in (300, 5000, 70000, 3)]
    qts = ["int8", "float16", "int8", "float16"]
    ys, _ = _fq_multi(ctx, arrays, qts)
    for a, y, q in zip(arrays, ys, qts):
        np.testing.assert_array_equal(_bits(y), _bits(fq_int8(a)[0] if q == "int8" else fq_f16(a)))


@pytest.mark.parametrize("shape", [(64, 128), (256, 32, 28, 28), (3, 5)])
@pytest.mark.parametrize("qtype", ["int8", "float16"])
def test_activation_kernel_bit_exact(ctx, shape, qtype):
    x = (np.random.default_rng(int(np.prod(shape))).standard_normal(shape) * 3).astype(f32)
    dx, dy, ds = ctx.upload(x), ctx.empty(x.size), ctx.empty(1)
    ctx.call("th_fake_quant_act", dx, dy, x.size, 0 if qtype == "int8" else 1, ds)
    y = ctx.download(dy, shape)
    if qtype == "int8":
        ref, scale = fq_act_int8(x)
        assert _bits(ctx.download(ds, (1,))).tolist() == _bits([scale]).tolist()
    else:
        ref = fq_f16(x)
    np.testing.assert_array_equal(_bits(y), _bits(ref))


def test_activation_kernel_edge_inputs(ctx):
    for name, x in _edge_inputs(np.random.default_rng(8)).items():
        dx, dy, ds = ctx.upload(x), ctx.empty(x.size), ctx.empty(1)
        ctx.call("th_fake_quant_act", dx, dy, x.size, 0, ds)
        ref, scale = fq_act_int8(x)
        np.testing.assert_array_equal(_bits(ctx.download(dy, x.shape)), _bits(ref), err_msg=name)
        assert _bits(ctx.download(ds, (1,))).tolist() == _bits([scale]).tolist(), name


def _off4_cases():
    rng = np.random.default_rng(11)
    cases = {f"n{n}": (rng.standard_normal(n) * 0.7).astype(f32) for n in (0, 1, 3, 4099, 256 * 1024 + 3)}
    cases.update(_edge_inputs(rng))
    return cases


@pytest.mark.parametrize("name", list(_off4_cases()))
def test_quant_kernels_on_unaligned_pointers(ctx, name):
    """th_quantize_int8, th_fake_quant_act (both codecs) and th_fake_quant_multi with every data pointer 4 bytes off a 16-byte boundary:
    the scalar walk of the shared span helper, bit for bit against the oracle's codecs (the item descriptors keep their 8-byte alignment)"""
    from taper_amd import hip as H
    a = _off4_cases()[name]
    n = a.size

    def down(ptr, dtype=f32):   # (length 0: the parameters only)
        return ctx.download(ptr, (n,), dtype) if n else np.empty(0, dtype)

    dx = ctx.upload(np.concatenate([np.zeros(1, f32), a]))   # (kept alive: x is dx.offset(4))
    x = dx.offset(4)
    assert x % 16 == 4

    q_ref, scale, _, mn = OX.quantize_int8(a)
    keep = [ctx.empty(n // 4 + 2), ctx.empty(3)]
    dq, dp = keep[0].offset(4), keep[1].offset(4)
    ctx.call("th_quantize_int8", x, dq, n, dp)
    assert _bits(ctx.download(dp, (2,))).tolist() == _bits([mn, scale]).tolist()
    np.testing.assert_array_equal(down(dq, np.int8), q_ref)

    for qtype, code in (("int8", 0), ("float16", 1)):
        keep = [ctx.empty(n + 2), ctx.empty(3)]
        dy, ds = keep[0].offset(4), keep[1].offset(4)
        ctx.call("th_fake_quant_act", x, dy, n, code, ds)
        ref, scale_ref = fq_act_int8(a) if qtype == "int8" else (fq_f16(a), f32(0))
        np.testing.assert_array_equal(_bits(down(dy)), _bits(ref), err_msg=qtype)
        assert _bits(ctx.download(ds, (1,))).tolist() == _bits([scale_ref]).tolist(), qtype

    keep = [ctx.empty(n + 2), ctx.empty(n + 2), ctx.empty(3), ctx.empty(3)]
    y8, y16, p8, p16 = (b.offset(4) for b in keep)
    for pp in (p8, p16):
        ctx.call("th_fill_f32", pp, float("nan"), 2)
    items = (H.FqItem * 2)(H.FqItem(x, y8, p8, n, 0), H.FqItem(x, y16, p16, n, 1))
    ctx.call("th_fake_quant_multi", ctx.upload(np.frombuffer(bytes(items), np.uint8)), 2)
    ref8, (mn8, scale8) = fq_int8(a)
    np.testing.assert_array_equal(_bits(down(y8)), _bits(ref8))
    assert _bits(ctx.download(p8, (2,))).tolist() == _bits([mn8, scale8]).tolist()
    np.testing.assert_array_equal(_bits(down(y16)), _bits(fq_f16(a)))


# ---------------------------------------------------------------- models
@pytest.fixture
def qat_on():
    import taper_amd as T
    T.qat.enable()
    T.qat.set_training_mode(True)
    yield T
    T.qat.disable()
    T.qat.set_training_mode(True)
    T.set_full_backward(False)


def _qat_model(T, spec, activations=False, qtype="int8"):
    cfg = T.QATConfig(qtype, activations=activations)
    layers = []
    for i, s in enumerate(spec):
        k = s["kind"]
        if k == "linear":
            o, n = s["w"].shape
            l = T.QATLinear(n, o, True, cfg, module_id=f"lin{i}")
        elif k == "conv2d_relu":
            co, ci, kh, kw = s["w"].shape
            l = T.QATConv2d(ci, co, (kh, kw), s.get("stride", (1, 1)), s.get("padding", (0, 0)), True, True, cfg, module_id=f"conv{i}")
        elif k == "relu":
            l = T.ReLU()
        elif k == "maxpool":
            l = T.MaxPool2d(s["kernel"], s.get("stride"), s.get("padding"))
        elif k == "adaptive_avgpool":
            l = T.AdaptiveAvgPool2d(s.get("out", (1, 1)))
        elif k == "flatten":
            l = T.Flatten(s.get("start_dim", 1))
        else:
            raise ValueError(k)
        if "w" in s:
            ps = l.parameters()
            ps[0].set_data(s["w"])
            ps[1].set_data(s["b"])
        layers.append(l)
    return T.Sequential(layers)


def _fq_spec(spec, qtype="int8"):
    out = []
    for s in spec:
        s = dict(s)
        for k in ("w", "b"):   # quantize() packs the bias too: QAT trains against its round trip as well
            if s.get(k) is not None:
                s[k] = (fq_int8(s[k])[0] if qtype == "int8" else fq_f16(s[k])).reshape(s[k].shape)
        out.append(s)
    return out


_ORACLE_RUNS = {}


def _oracle_qat_run(spec, x, y, shape, batch, steps, lr, full_backward):
    """fake-quantize the weights in numpy, run the oracle's step on them, apply Adam (optim.rs:83-113) to the master weights"""
    masters = [O.Tensor(s[k]).requires_grad() for s in spec if "w" in s for k in ("w", "b")]
    opt = O.Adam(masters, lr)
    ob = backends.OracleBackend()
    losses = []
    for st in range(steps):
        cur, it = [], iter(masters)
        for s in spec:
            s = dict(s)
            if "w" in s:
                s["w"], s["b"] = next(it).data().reshape(s["w"].shape), next(it).data()
            cur.append(s)
        model = ob.sequential(_fq_spec(cur), full_backward=full_backward)
        sl = slice(st * batch, (st + 1) * batch)
        loss, _, _, grads = ob.forward_backward(model, x[sl], y[sl], (batch, *shape))
        losses.append(loss)
        for m, g in zip(masters, grads):
            if g is not None and len(g):
                m.set_grad(np.asarray(g, f32).reshape(-1))
        opt.step()
        opt.zero_grad()
    return [m.data() for m in masters], losses


def _grads_hip(T, model, x, y, shape):
    T.Tape.reset()
    logits = model.forward(T.Tensor(x, (x.shape[0], *shape)))
    loss = T.cross_entropy_loss(logits, T.Tensor(y))
    loss.backward()
    gs = [p.grad() for p in model.parameters()]
    for p in model.parameters():
        p.zero_grad()
    T.Tape.reset()
    return float(loss.data()[0]), gs


@pytest.mark.parametrize("name,full_backward", [("mlp_baseline", False), ("cnn_simple", False), ("cnn_simple", True)])
def test_straight_through_estimator_grads(qat_on, name, full_backward):
    T = qat_on
    build, shape = (backends.mlp_baseline, (784,)) if name == "mlp_baseline" else (backends.cnn_simple, (1, 28, 28))
    rng = np.random.default_rng(21)
    spec = backends.nonzero_biases(build(rng), rng)
    x, y = backends.mnist_like(rng, 32)
    T.set_full_backward(full_backward)
    model = _qat_model(T, spec)
    loss, gs = _grads_hip(T, model, x, y, shape)
    ob = backends.OracleBackend()
    rloss, _, _, rgs = ob.forward_backward(ob.sequential(_fq_spec(spec), full_backward=full_backward), x, y, (32, *shape))
    assert abs(loss - rloss) <= RTOL * max(1.0, abs(rloss))
    for g, r in zip(gs, rgs):
        if r is None or len(r) == 0:
            assert g is None or len(g) == 0 or not np.any(g)
            continue
        assert _err(np.asarray(g).reshape(-1), np.asarray(r).reshape(-1)) <= RTOL
    # Adam updates the masters; the next forward's round trips are made from them
    ps0 = [p.data().copy() for p in model.parameters()]
    opt = T.Adam(model.parameters(), 1e-3)
    T.Trainer(model, opt, sample_shape=shape if len(shape) > 1 else None).train_step(T.Tensor(x, (32, 784)), T.Tensor(y))
    ps1 = [p.data().copy() for p in model.parameters()]
    moved = [i for i, r in enumerate(rgs) if r is not None and len(r) and np.any(r)]
    assert moved and all(np.abs(ps1[i] - ps0[i]).max() > 1e-5 for i in moved)
    model.forward(T.Tensor(x, (32, *shape)))
    first = model.layers[0]
    np.testing.assert_array_equal(_bits(first.fake_quantized("weight").data()), _bits(fq_int8(ps1[0])[0]))
    np.testing.assert_array_equal(_bits(first.fake_quantized("bias").data()), _bits(fq_int8(ps1[1])[0]))


@pytest.mark.parametrize("mode", ["eager", "graph_fused", "graph_unfused"])
@pytest.mark.parametrize("name,batch,full_backward", [("mlp_baseline", 64, False), ("cnn_simple", 256, False)])
def test_training_loop_matches_oracle(qat_on, name, batch, full_backward, mode):
    T = qat_on
    build, shape = (backends.mlp_baseline, (784,)) if name == "mlp_baseline" else (backends.cnn_simple, (1, 28, 28))
    rng = np.random.default_rng(31)
    spec = backends.nonzero_biases(build(rng), rng)
    steps, lr = 20, 1e-3
    x, y = backends.mnist_like(rng, steps * batch)
    T.set_full_backward(full_backward)
    model = _qat_model(T, spec)
    opt = T.Adam(model.parameters(), lr)
    tr = T.Trainer(model, opt, sample_shape=shape if len(shape) > 1 else None, fuse_adam=(mode != "graph_unfused"))
    loader = T.DataLoader(T.MNISTDataset.from_host(x, y), batch, False)
    r = tr.train_epoch(loader) if mode == "eager" else tr.train_epoch_graph(loader)
    key = (name, batch, full_backward)
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = _oracle_qat_run(spec, x, y, shape, batch, steps, lr, full_backward)
    ref, rlosses = _ORACLE_RUNS[key]
    np.testing.assert_allclose(r["losses"], rlosses, rtol=RTOL, atol=RTOL)
    for p, q in zip(model.parameters(), ref):
        assert _err(p.data().reshape(-1), q.reshape(-1)) <= RTOL


@pytest.mark.parametrize("mode", ["eager", "graph_fused", "graph_unfused"])
def test_full_backward_steps_match_oracle(qat_on, mode):
    """The simple CNN at B = 256 in full-backward mode, where the conv weights train too: 20 steps, each checked against the oracle's step
    (numpy fake-quant, oracle forward / backward, Adam on the masters) from the SAME master weights.  (Over a whole run the two would
    part: the conv weight gradients sum in another order, the masters differ in the last bits, and a weight that sits on a rounding
    boundary of the int8 codec then takes the neighbouring code -- a 1/255-of-range step, not an error of either side.)  The captured
    modes run each step as a one-batch epoch of train_epoch_graph."""
    T = qat_on
    rng = np.random.default_rng(81)
    spec = backends.nonzero_biases(backends.cnn_simple(rng), rng)
    B, steps, lr, shape = 256, 20, 1e-3, (1, 28, 28)
    x, y = backends.mnist_like(rng, steps * B)
    T.set_full_backward(True)
    model = _qat_model(T, spec)
    tr = T.Trainer(model, T.Adam(model.parameters(), lr), sample_shape=shape, fuse_adam=(mode != "graph_unfused"))
    masters = [O.Tensor(p.data().reshape(-1)).requires_grad() for p in model.parameters()]
    oopt = O.Adam(masters, lr)
    ob = backends.OracleBackend()
    for st in range(steps):
        sl = slice(st * B, (st + 1) * B)
        state = [p.data() for p in model.parameters()]
        for m, v in zip(masters, state):
            m.set_data(v.reshape(-1))
        cur, it = [], iter(state)
        for s in spec:
            s = dict(s)
            if "w" in s:
                s["w"], s["b"] = next(it).reshape(s["w"].shape), next(it)
            cur.append(s)
        rloss, _, _, grads = ob.forward_backward(ob.sequential(_fq_spec(cur), full_backward=True), x[sl], y[sl], (B, *shape))
        for m, g in zip(masters, grads):
            m.set_grad(np.asarray(g, f32).reshape(-1))
        oopt.step()
        oopt.zero_grad()
        if mode == "eager":
            loss = tr.train_step(T.Tensor(x[sl], (B, 784)), T.Tensor(y[sl]))[0]
        else:
            loss = float(tr.train_epoch_graph(T.DataLoader(T.MNISTDataset.from_host(x[sl], y[sl]), B, False))["losses"][0])
        assert abs(loss - rloss) <= RTOL * max(1.0, abs(rloss)), (st, loss, rloss)
        for p, m in zip(model.parameters(), masters):
            assert _err(p.data().reshape(-1), m.data()) <= RTOL, st


def test_activation_fake_quant_training(qat_on):
    """5 steps of a small QAT MLP with activation fake-quant against a numpy forward / backward of the same model"""
    T = qat_on
    rng = np.random.default_rng(41)
    spec = backends.nonzero_biases([backends._lin(rng, 784, 32), dict(kind="relu"), backends._lin(rng, 32, 10)], rng)
    B, steps, lr = 16, 5, 1e-3
    x, y = backends.mnist_like(rng, steps * B)
    model = _qat_model(T, spec, activations=True)
    opt = T.Adam(model.parameters(), lr)
    tr = T.Trainer(model, opt)
    hip_losses = [tr.train_step(T.Tensor(x[s * B:(s + 1) * B], (B, 784)), T.Tensor(y[s * B:(s + 1) * B]))[0] for s in range(steps)]
    w = [spec[0]["w"].copy(), spec[0]["b"].copy(), spec[2]["w"].copy(), spec[2]["b"].copy()]
    masters = [O.Tensor(a).requires_grad() for a in w]
    oopt = O.Adam(masters, lr)
    for s in range(steps):
        xb, yb = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B].astype(np.int64)
        W1, b1, W2, b2 = [fq_int8(m.data())[0] for m in masters]
        q1, q2 = W1.reshape(32, 784), W2.reshape(10, 32)
        z1 = fq_act_int8((xb.astype(np.float64) @ q1.T.astype(np.float64) + b1).astype(f32))[0]
        h = np.maximum(z1, 0)
        z2 = fq_act_int8((h.astype(np.float64) @ q2.T.astype(np.float64) + b2).astype(f32))[0].astype(np.float64)
        z2 -= z2.max(1, keepdims=True)
        p = np.exp(z2) / np.exp(z2).sum(1, keepdims=True)
        loss = float(-np.log(p[np.arange(B), yb]).mean())
        assert abs(loss - hip_losses[s]) <= 1e-4 * max(1.0, loss), (s, loss, hip_losses[s])
        d2 = p.copy()
        d2[np.arange(B), yb] -= 1
        d2 /= B
        dh = (d2 @ q2.astype(np.float64)) * (z1 > 0)
        grads = [dh.T @ xb, dh.sum(0), d2.T @ h, d2.sum(0)]
        for m, g in zip(masters, grads):
            m.set_grad(np.asarray(g, f32).reshape(-1))
        oopt.step()
        oopt.zero_grad()
    for pp, m in zip(model.parameters(), masters):
        assert _err(pp.data().reshape(-1), m.data().reshape(-1)) <= 1e-3
    obs = model.layers[0].observed()
    assert obs["weight_scale"] > 0 and obs["activation_scale"] > 0


@pytest.mark.parametrize("name", ["mlp_baseline", "cnn_simple"])
def test_deployment_packs_the_trained_fake_quantized_weights(qat_on, name):
    T = qat_on
    build, shape = (backends.mlp_baseline, (784,)) if name == "mlp_baseline" else (backends.cnn_simple, (1, 28, 28))
    rng = np.random.default_rng(51)
    spec = backends.nonzero_biases(build(rng), rng)
    B = 64
    x, y = backends.mnist_like(rng, 5 * B)
    model = _qat_model(T, spec)
    tr = T.Trainer(model, T.Adam(model.parameters(), 1e-3), sample_shape=shape if len(shape) > 1 else None)
    tr.train_epoch_graph(T.DataLoader(T.MNISTDataset.from_host(x, y), B, False))
    xt = T.Tensor(x[:B], (B, *shape))
    qat_out = model.forward(xt).data()    # training mode: this forward fake-quantizes the current masters
    q = model.quantize("int8")
    ts = q.tensors()
    qat_layers = [l for l in model.layers if isinstance(l, (T.QATLinear, T.QATConv2d))]
    for i, l in enumerate(qat_layers):
        for j, which in enumerate(("weight", "bias")):
            kind, codes, (mn, scale) = ts[2 * i + j]
            np.testing.assert_array_equal(_bits(OX.dequantize_int8(codes, scale, -128, mn)), _bits(l.fake_quantized(which).data().reshape(-1)))
    got = q(xt).data()
    assert _err(got, qat_out) <= 1e-5


@pytest.mark.parametrize("name", ["mlp_baseline", "cnn_simple"])
def test_inactive_forward_is_the_plain_twin(qat_on, name):
    T = qat_on
    build, shape = (backends.mlp_baseline, (784,)) if name == "mlp_baseline" else (backends.cnn_simple, (1, 28, 28))
    rng = np.random.default_rng(61)
    spec = backends.nonzero_biases(build(rng), rng)
    x = rng.uniform(0, 1, (8, 784)).astype(f32)
    twin = backends.HipBackend().sequential(spec).forward(T.Tensor(x, (8, *shape))).data()
    model = _qat_model(T, spec, activations=True)
    xt = T.Tensor(x, (8, *shape))
    assert not np.array_equal(_bits(model.forward(xt).data()), _bits(twin))   # active: fake-quantized
    T.qat.disable()
    np.testing.assert_array_equal(_bits(model.forward(xt).data()), _bits(twin))
    T.qat.enable()
    T.qat.set_training_mode(False)
    np.testing.assert_array_equal(_bits(model.forward(xt).data()), _bits(twin))
    T.qat.set_training_mode(True)
    for l in model.layers:
        if isinstance(l, (T.QATLinear, T.QATConv2d)):
            l.enable_qat(False)
    np.testing.assert_array_equal(_bits(model.forward(xt).data()), _bits(twin))
    st = T.qat.status()
    assert st["global_enabled"] and st["training_mode"] and st["enabled_modules"] < st["module_count"]
    for l in model.layers:
        if isinstance(l, (T.QATLinear, T.QATConv2d)):
            l.enable_qat(True)


def test_mode_switch_rerecords_the_graphs(qat_on):
    """QAT on for one captured epoch, training mode off for the next: the second epoch is eager f32 training from the same state, bit for
    bit (a replay of the first epoch's graphs would still fake-quantize)"""
    T = qat_on
    rng = np.random.default_rng(71)
    spec = backends.nonzero_biases(backends.mlp_baseline(rng), rng)
    B = 64
    x, y = backends.mnist_like(rng, 8 * B)
    model = _qat_model(T, spec)
    opt = T.Adam(model.parameters(), 1e-3)
    tr = T.Trainer(model, opt)
    loader = T.DataLoader(T.MNISTDataset.from_host(x, y), B, False)
    tr.train_epoch_graph(loader)
    state = [p.data().copy() for p in model.parameters()]
    path = Path(__import__("tempfile").mkdtemp()) / "adam.txt"
    tr.save_optimizer_state(path)

    def restore(t):
        for p, v in zip(model.parameters(), state):
            p.set_data(v)
        t.load_optimizer_state(path)

    qat_losses = tr.train_epoch_graph(loader)["losses"]   # (the same graphs, replayed from the snapshot's successor state)
    restore(tr)
    T.qat.set_training_mode(False)
    r = tr.train_epoch_graph(loader)
    got = [p.data().copy() for p in model.parameters()]
    fresh = T.Trainer(model, opt)
    restore(fresh)
    rp = fresh.train_epoch(loader)
    np.testing.assert_array_equal(_bits(r["losses"]), _bits(rp["losses"]))
    for a, p in zip(got, model.parameters()):
        np.testing.assert_array_equal(_bits(a), _bits(p.data()))
    assert not np.array_equal(_bits(r["losses"]), _bits(qat_losses))
    T.qat.set_training_mode(True)


def test_eager_step_between_graph_epochs_rerecords(qat_on):
    """captured epoch with every layer active; one layer off for an eager train_step (a new descriptor list: the buffer the graphs read is
    replaced and freed); the layer back on, so the switches equal the first epoch's again; the next captured epoch must not replay the
    old graphs -- it equals the same epoch run eagerly from the same state, bit for bit"""
    T = qat_on
    rng = np.random.default_rng(91)
    spec = backends.nonzero_biases(backends.mlp_baseline(rng), rng)
    B = 64
    x, y = backends.mnist_like(rng, 8 * B)
    model = _qat_model(T, spec)
    opt = T.Adam(model.parameters(), 1e-3)
    tr = T.Trainer(model, opt)
    loader = T.DataLoader(T.MNISTDataset.from_host(x, y), B, False)
    tr.train_epoch_graph(loader)
    first = model.layers[0]
    first.enable_qat(False)
    tr.train_step(T.Tensor(x[:B], (B, 784)), T.Tensor(y[:B]))
    first.enable_qat(True)
    state = [p.data().copy() for p in model.parameters()]
    path = Path(__import__("tempfile").mkdtemp()) / "adam.txt"
    tr.save_optimizer_state(path)
    r = tr.train_epoch_graph(loader)
    got = [p.data().copy() for p in model.parameters()]
    fresh = T.Trainer(model, opt)
    for p, v in zip(model.parameters(), state):
        p.set_data(v)
    fresh.load_optimizer_state(path)
    rp = fresh.train_epoch(loader)
    np.testing.assert_array_equal(_bits(r["losses"]), _bits(rp["losses"]))
    for a, p in zip(got, model.parameters()):
        np.testing.assert_array_equal(_bits(a), _bits(p.data()))


def test_shared_qat_layer_is_refused(qat_on):
    T = qat_on
    head, shared, tail = T.QATLinear(784, 16), T.QATLinear(16, 16, module_id="shared"), T.QATLinear(16, 10)
    model = T.Sequential([head, T.ReLU(), shared, T.ReLU(), shared, T.ReLU(), tail])
    tr = T.Trainer(model, T.Adam(head.parameters() + shared.parameters() + tail.parameters(), 1e-3))
    x, y = backends.mnist_like(np.random.default_rng(2), 64)
    with pytest.raises(T.TaperError, match="same QAT layer twice"):
        tr.train_epoch_graph(T.DataLoader(T.MNISTDataset.from_host(x, y), 64, False))
    with pytest.raises(T.TaperError, match="same QAT layer twice"):
        tr.train_step(T.Tensor(x, (64, 784)), T.Tensor(y))


def test_data_parallel_qat_is_refused(qat_on):
    T = qat_on
    model = T.Sequential([T.QATLinear(784, 16), T.ReLU(), T.QATLinear(16, 10)])
    tr = T.Trainer(model, T.Adam(model.parameters(), 1e-3), comm=T.Communicator.loopback())
    x, y = backends.mnist_like(np.random.default_rng(1), 32)
    with pytest.raises(T.TaperError, match="data-parallel"):
        tr.train_step(T.Tensor(x, (32, 784)), T.Tensor(y))


def test_qat_example_prints_both_accuracies_and_sizes():
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "examples")])
    for model in ("cnn", "mlp"):
        out = subprocess.run([str(ROOT / "examples" / "_build" / "qat_train"), "--data-dir", "/nonexistent", "--model", model, "--steps", "5",
                              "--train-n", "512", "--test-n", "256"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr + out.stdout
        for pat in (r"QAT model accuracy \(eval\): [\d.]+%", r"Int8 model accuracy: [\d.]+%", r"Float32 size: \d+ bytes", r"Int8 size: \d+ bytes"):
            assert re.search(pat, out.stdout), (pat, out.stdout)
        f32s = int(re.search(r"Float32 size: (\d+) bytes", out.stdout).group(1))
        i8s = int(re.search(r"Int8 size: (\d+) bytes", out.stdout).group(1))
        assert i8s < f32s / 3
