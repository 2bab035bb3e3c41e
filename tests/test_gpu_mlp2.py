"""th_mlp2_xent -- the large-batch step of Linear + ReLU, Linear, softmax cross-entropy in three launches (rows / dW1 K slices / fixed-order
finish with Adam), reading the batch's rows through the loader's index vector -- against the oracle's unfused chain
(/root/reference/src/nn.rs:54-60, src/loss.rs:101-195, 271-290, src/ops.rs:238-294, 358-369, src/tensor.rs:574-587, 674-694,
src/optim.rs:83-113, src/data/mnist.rs:277-310)."""
import ctypes as C

import numpy as np
import pytest

from tests import margins
from tests.test_gpu_fused import _adam_ref, close, RTOL
from tests.test_gpu_mlp_tail import oracle_tail
from taper_amd.hip import AdamFuse, RowSource

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _params(rng, inf, hid, c):
    w1 = rng.uniform(-1, 1, (hid, inf)).astype(np.float32) * np.float32(np.sqrt(2.0 / inf))
    b1 = rng.uniform(-0.1, 0.1, hid).astype(np.float32)
    w2 = rng.uniform(-0.3, 0.3, (c, hid)).astype(np.float32)
    b2 = rng.uniform(-0.1, 0.1, c).astype(np.float32)
    return w1, b1, w2, b2


def _call(ctx, src, batch, inf, hid, c, dev, fuses=(None, None, None, None), tick=None, log=None):
    out = dict(dw1=ctx.empty(hid * inf), db1=ctx.empty(hid), dw2=ctx.empty(c * hid), db2=ctx.empty(c), loss=ctx.empty(1), nc=ctx.empty(1))
    metrics, cap, state, adv = log if log else (None, 0, None, 0)
    ctx.call("th_mlp2_xent", C.byref(src), batch, inf, hid, c, dev["w1"], dev["b1"], dev["w2"], dev["b2"], out["dw1"], out["db1"], out["dw2"],
             out["db2"], out["loss"], out["nc"], metrics, cap, state, adv, tick, *[C.byref(f) if f is not None else None for f in fuses])
    return out


def _check_grads(ctx, out, ref, inf, hid, c, name):
    loss = ctx.download(out["loss"], 1)[0]
    assert loss == pytest.approx(ref["loss"], rel=RTOL, abs=1e-6)
    assert ctx.download(out["nc"], 1)[0] == ref["ncorrect"]                 # index work: exact
    for k, shape in (("dw1", (hid, inf)), ("db1", (hid,)), ("dw2", (c, hid)), ("db2", (c,))):
        got = ctx.download(out[k], shape)
        close(got, np.asarray(ref[k]).reshape(shape), atol=1e-6)
        margins.check(f"{k}", got, np.asarray(ref[k]).reshape(shape), 1e-4, test=name)


# (hidden widths that are not multiples of 32 -- 100, 20, 4, 116 -- end inside a wave's 16-column tile: r05)
DENSE = [(1024, 784, 128, 10), (4096, 784, 128, 10), (1000, 100, 64, 5), (33, 36, 32, 16), (5000, 784, 96, 10), (2048, 64, 128, 3),
         (12288 + 5, 784, 128, 10), (16384, 784, 128, 10), (2048, 784, 100, 10), (520, 64, 20, 4), (700, 100, 4, 3), (4100, 784, 116, 10),
         (13000, 784, 100, 10)]


@pytest.mark.parametrize("batch,inf,hid,c", DENSE)
def test_mlp2_dense_rows(ctx, O, batch, inf, hid, c):
    rng = np.random.default_rng(batch + inf + hid + c)
    x = (rng.integers(0, 256, (batch, inf)) * (rng.uniform(0, 1, (batch, inf)) < 0.3)).astype(np.float32) / np.float32(255.0)
    y = rng.integers(0, c, batch).astype(np.float32)
    w1, b1, w2, b2 = _params(rng, inf, hid, c)
    ref = oracle_tail(O, x, w1, b1, w2, b2, y)
    dev = dict(w1=ctx.upload(w1), b1=ctx.upload(b1), w2=ctx.upload(w2), b2=ctx.upload(b2))
    dx, dy = ctx.upload(x), ctx.upload(y)
    src = RowSource(int(dx), int(dy), None, None, 0, batch)
    calls = C.c_int64()
    from taper_amd._lib import hip as lib
    lib.th_debug_mlp2_calls(C.byref(calls))
    out = _call(ctx, src, batch, inf, hid, c, dev)
    _check_grads(ctx, out, ref, inf, hid, c, "test_mlp2_dense_rows")
    after = C.c_int64()
    lib.th_debug_mlp2_calls(C.byref(after))
    assert after.value == calls.value + 1
    # deterministic: fixed-order sums, no atomics
    out2 = _call(ctx, src, batch, inf, hid, c, dev)
    for k, n in (("dw1", hid * inf), ("dw2", c * hid), ("db1", hid), ("db2", c), ("loss", 1)):
        np.testing.assert_array_equal(ctx.download(out[k], n), ctx.download(out2[k], n))
    for k, a in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):          # parameters are only read without a fuse
        np.testing.assert_array_equal(ctx.download(dev[k], a.shape), a)


@pytest.mark.parametrize("n_rows,batch,cursor", [(3000, 256, 0), (3000, 256, 2900), (5000, 2048, 4000), (60000, 4096, 57000)])
def test_mlp2_rows_through_the_index_vector(ctx, O, n_rows, batch, cursor):
    """rows idx[(cursor + r) % n] of a resident dataset (data/mnist.rs:277-310 without the copy), wrapping at the epoch's end"""
    inf, hid, c = 784, 128, 10
    rng = np.random.default_rng(n_rows + batch + cursor)
    data = (rng.integers(0, 256, (n_rows, inf)) * (rng.uniform(0, 1, (n_rows, inf)) < 0.25)).astype(np.float32) / np.float32(255.0)
    labels = rng.integers(0, c, n_rows).astype(np.float32)
    idx = rng.permutation(n_rows).astype(np.int32)
    rows = idx[(cursor + np.arange(batch)) % n_rows]
    w1, b1, w2, b2 = _params(rng, inf, hid, c)
    ref = oracle_tail(O, data[rows], w1, b1, w2, b2, labels[rows])
    dev = dict(w1=ctx.upload(w1), b1=ctx.upload(b1), w2=ctx.upload(w2), b2=ctx.upload(b2))
    dd, dl, di = ctx.upload(data), ctx.upload(labels), ctx.upload(idx)
    state = ctx.upload(np.array([3, cursor], np.int64))
    src = RowSource(int(dd), int(dl), int(di), state.offset(8), n_rows, n_rows)
    metrics = ctx.zeros(2 * 8)
    out = _call(ctx, src, batch, inf, hid, c, dev, log=(metrics, 8, state, batch))
    _check_grads(ctx, out, ref, inf, hid, c, "test_mlp2_rows_through_the_index_vector")
    # the step log (train.rs:117-121): slot state[0], then step += 1, cursor += batch
    np.testing.assert_array_equal(ctx.download(state, 2, np.int64), [4, cursor + batch])
    m = ctx.download(metrics, 16)
    assert m[6] == ctx.download(out["loss"], 1)[0] and m[7] == ref["ncorrect"]
    # bit-identical to the same rows handed over as a dense block
    dx, dy = ctx.upload(data[rows]), ctx.upload(labels[rows])
    out_d = _call(ctx, RowSource(int(dx), int(dy), None, None, 0, batch), batch, inf, hid, c, dev)
    for k, n in (("dw1", hid * inf), ("dw2", c * hid), ("db1", hid), ("db2", c), ("loss", 1), ("nc", 1)):
        np.testing.assert_array_equal(ctx.download(out[k], n), ctx.download(out_d[k], n))


@pytest.mark.parametrize("batch,inf,hid,c", [(1024, 784, 128, 10), (4096, 784, 128, 10), (1500, 100, 64, 7)])
def test_mlp2_adam_in_the_finish_launch(ctx, O, batch, inf, hid, c):
    """launch 1 opens the optimizer step (t += 1, optim.rs:84); launch 3 applies optim.rs:99-110 at that t to all four parameters"""
    rng = np.random.default_rng(batch * 3 + hid)
    x = rng.uniform(0, 1, (batch, inf)).astype(np.float32)
    y = rng.integers(0, c, batch).astype(np.float32)
    w1, b1, w2, b2 = _params(rng, inf, hid, c)
    ref = oracle_tail(O, x, w1, b1, w2, b2, y)
    lr, t = 1e-3, 6
    dev = dict(w1=ctx.upload(w1), b1=ctx.upload(b1), w2=ctx.upload(w2), b2=ctx.upload(b2))
    mom = {k: (ctx.zeros(v.size), ctx.zeros(v.size)) for k, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))}
    tick, dlr = ctx.upload(np.array([t, 0], np.int32)), ctx.upload(np.array([lr], np.float32))
    fuses = [AdamFuse(int(dev[k]), int(mom[k][0]), int(mom[k][1]), int(tick), int(dlr), 0.9, 0.999, 1e-8, 1e-4) for k in ("w1", "b1", "w2", "b2")]
    dx, dy = ctx.upload(x), ctx.upload(y)
    out = _call(ctx, RowSource(int(dx), int(dy), None, None, 0, batch), batch, inf, hid, c, dev, fuses=fuses, tick=tick)
    assert ctx.download(tick, 2, np.int32)[0] == t + 1
    _check_grads(ctx, out, ref, inf, hid, c, "test_mlp2_adam_in_the_finish_launch")
    for k, p0, g in (("w1", w1, ref["dw1"]), ("b1", b1, ref["db1"]), ("w2", w2, ref["dw2"]), ("b2", b2, ref["db2"])):
        p_ref, m_ref, v_ref = _adam_ref(O, p0.reshape(-1), np.asarray(g, np.float32).reshape(-1), lr, t + 1)
        margins.check(f"{k}_after_adam", ctx.download(dev[k], p0.size), p_ref, 2e-2, lr=lr)      # (the smoke's error model: 2 % of lr)
        margins.check(f"{k}_m", ctx.download(mom[k][0], p0.size), m_ref, 1e-4)
        margins.check(f"{k}_v", ctx.download(mom[k][1], p0.size), v_ref, 2e-4)


def test_mlp2_out_of_range_target_raises(ctx):
    from taper_amd._lib import TaperError
    rng = np.random.default_rng(5)
    batch, inf, hid, c = 1024, 784, 128, 10
    x = rng.uniform(0, 1, (batch, inf)).astype(np.float32)
    y = rng.integers(0, c, batch).astype(np.float32)
    y[700] = 12.0
    w1, b1, w2, b2 = _params(rng, inf, hid, c)
    dev = dict(w1=ctx.upload(w1), b1=ctx.upload(b1), w2=ctx.upload(w2), b2=ctx.upload(b2))
    dx, dy = ctx.upload(x), ctx.upload(y)
    _call(ctx, RowSource(int(dx), int(dy), None, None, 0, batch), batch, inf, hid, c, dev)
    with pytest.raises(TaperError, match="Target class 12 out of bounds for 10"):
        ctx.sync()


def _mlp2_calls():
    from taper_amd._lib import hip as lib
    n = C.c_int64()
    lib.th_debug_mlp2_calls(C.byref(n))
    return n.value


@pytest.mark.parametrize("n,batch,shuffle,model", [(10000, 4096, True, "mlp_baseline"), (40000, 16384, True, "mlp_baseline"), (8192, 4096, False, "mlp_baseline"),
                                                   (20000, 20000, False, "mlp_baseline"),
                                                   # examples/train_mnist.rs:40-48's own model (two hidden layers) through th_mlp2_xent_deep
                                                   (10000, 4096, True, "mlp_example"), (40000, 16384, True, "mlp_example"), (5000, 2048, True, "mlp_example"),
                                                   # hidden widths that are no multiples of 32 / 16 take the same step (ragged tiles)
                                                   (10000, 4096, True, "mlp_100"), (3000, 1024, True, "mlp_100_52")])
def test_trainer_large_batch_epochs_match_oracle(n, batch, shuffle, model):
    """Trainer steps of the MNIST MLP at batch >= 2048 take th_mlp2_xent: the rows are read in place through the loader's index vector (a
    last partial batch below 2048 rows is gathered and takes the small-batch forms).  Two epochs (graph replay: the second reuses the
    captured steps on reshuffled data) against the oracle's loop fed by a twin loader with the same seed."""
    import taper_amd as T
    from tests import backends
    H, Orc = backends.get("hip"), backends.get("oracle")
    Orc.set_zero_sentinel(True)
    rng = np.random.default_rng(n + batch)
    spec = backends.nonzero_biases(getattr(backends, model)(rng), rng)
    x, y = backends.mnist_like(rng, n)
    hm, om = H.sequential(spec), Orc.sequential(spec)
    lr = 1e-3
    hopt, oopt = T.Adam(hm.parameters(), lr, None, None, 1e-4), Orc.m.Adam(om.parameters(), lr, None, None, 1e-4)
    tr = T.Trainer(hm, hopt)
    ds = T.MNISTDataset.from_host(x, y)
    loader, twin = T.DataLoader(ds, batch, shuffle, seed=77), T.DataLoader(ds, batch, shuffle, seed=77)
    before = _mlp2_calls()
    n_big = 0
    for epoch in range(2):
        ep = tr.run_epoch(loader, T.Trainer.GRAPH)
        twin.reset()
        ref_losses, ref_nc = [], []
        for xb, yb in twin:
            xb, yb = xb.data(), yb.data()
            r = om.train_step(oopt, xb, yb, xb.shape)
            ref_losses.append(r["loss"])
            ref_nc.append(round(r["acc"] * len(yb)))
            n_big += 1 if len(yb) >= 480 else 0
        margins.check(f"losses_epoch{epoch}", ep["losses"], ref_losses, 4e-6)      # observed <= 1.6e-6 of the largest (r04)
        assert np.abs(ep["ncorrect"] - np.array(ref_nc)).max() <= 3                   # an argmax between two logits within rounding may flip (16 384 rows of an untrained net: 2 seen)
    assert _mlp2_calls() - before >= 1 and n_big >= 2                                 # (captured steps replay without new enqueues)
    assert hopt.t() == oopt.t()
    # Adam moves a weight by lr * m / (sqrt(v) + eps) per step: for the few W1 elements whose gradient is a sum of 16 384 terms cancelling to
    # ~eps, a reordered sum changes the step by a few % of lr (the smoke's error model: 2 % of lr per step), and the steps' errors add:
    # observed 7.1e-2 lr after 6 steps (b1 5.5e-3, W2 5.3e-4, b2 3.7e-5); the gradients themselves agree to 3e-6 of their scale (above)
    # (elements whose gradient stands clear of eps: sqrt(v) > 1e-5; every element within 2 lr per step -- tests/margins.py.  The two-hidden-
    # layer model has more of the near-eps elements: 1.3 lr seen on one of W1's after 6 steps at 16 384 rows)
    for i, (hp, op) in enumerate(zip(hm.parameters(), om.parameters())):
        # (two hidden layers: a second layer of ReLU masks between W1 / W2 and the loss -- 3.1e-2 lr per step seen on W2 at 16 384 rows)
        margins.check_adam_weights(f"{model}_param{i}", hp.data(), op.data(), oopt.v(i), lr, hopt.t(), (2e-2 if model == "mlp_baseline" else 6e-2) * hopt.t())
    T.Tape.reset()


def test_trainer_large_batch_graph_equals_eager_launches():
    """the captured steps (hipGraph replay of th_mlp2_xent) and Trainer.EAGER (the reference-literal loop on the launch-per-layer kernels)
    agree within fp32 reordering; the mlp2 form itself is deterministic run to run.  Adam's eps is 1e-3 here, not the default 1e-8: with
    the default, an element whose gradient is below the paths' ~1e-8 of absolute rounding error moves by +-lr per step on noise alone
    (optim.rs:104-109: m_hat / (sqrt(v_hat) + eps)), and one hidden pre-activation within rounding of zero (a ReLU mask flip, ~0.5 expected
    per 4096 x 128 step) shifts a whole W1 row's small gradients by ~1e-5 -- measured on this very case: W1 up to 1.9 lr apart at
    eps = 1e-8, 0.14 lr (one row) at 1e-5, 6e-4 lr at 1e-3, while each path's one-step gradients sit within 1.3e-8 of the oracle's.  At
    eps = 1e-3 the comparison is about the kernels: a wrong element would still show as >> 1e-3 lr.  (Default-eps weights are held to
    the oracle in test_trainer_large_batch_epochs_match_oracle.)"""
    import taper_amd as T
    from tests import backends
    H = backends.get("hip")
    rng = np.random.default_rng(9)
    spec = backends.nonzero_biases(backends.mlp_baseline(rng), rng)
    n, batch = 12288, 4096
    x, y = backends.mnist_like(rng, n)
    outs = []
    for mode in (T.Trainer.GRAPH, T.Trainer.GRAPH, T.Trainer.EAGER):
        model = H.sequential(spec)
        opt = T.Adam(model.parameters(), 1e-3, None, 1e-3, 1e-4)
        tr = T.Trainer(model, opt)
        loader = T.DataLoader(T.MNISTDataset.from_host(x, y), batch, True, seed=5)
        ep = [tr.run_epoch(loader, mode) for _ in range(2)]
        outs.append((np.concatenate([e["losses"] for e in ep]), [p.data() for p in model.parameters()]))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        np.testing.assert_array_equal(a, b)
    margins.check("losses_graph_vs_eager", outs[0][0], outs[2][0], 1e-5)
    for i, (a, b) in enumerate(zip(outs[0][1], outs[2][1])):
        margins.check(f"param{i}_graph_vs_eager", a, b, 1.5e-3, lr=1e-3)
    T.Tape.reset()


@pytest.mark.parametrize("form,ksplit", [("dense", 1), ("dense", 3), ("index", 1), ("index", 3)])
def test_mlp2_forced_ksplit(ctx, O, form, ksplit):
    """the 16-row tiles with a row block's k chunks on one workgroup and on three (th_debug_mlp2_ksplit; at 1 024 / 2 048 rows the launcher
    itself splits by 4 / 2), dense rows and rows through the index vector, against the oracle"""
    from taper_amd._lib import hip as lib
    lib.th_debug_mlp2_ksplit(ksplit)
    try:
        if form == "dense":
            test_mlp2_dense_rows(ctx, O, 1024, 784, 128, 10)
        else:
            test_mlp2_rows_through_the_index_vector(ctx, O, 5000, 2048, 4000)
    finally:
        lib.th_debug_mlp2_ksplit(0)


# ------------------------------------------------------------------------------------------------------------------ two hidden layers
def _oracle3(O, x, y, net):
    """reference chain of examples/train_mnist.rs:40-48: Linear + ReLU, Linear + ReLU, Linear, cross_entropy_loss; backward from the loss"""
    O.Tape.reset()
    O.Tape.set_zero_sentinel(True)
    params = [(O.Tensor(w).requires_grad(), O.Tensor(b).requires_grad()) for w, b in net]
    h = O.Tensor(x)
    for i, (w, b) in enumerate(params):
        h = h.matmul(w.transpose()).add_broadcast(b)
        if i < 2:
            h = h.relu()
    yt = O.Tensor(y)
    loss = O.cross_entropy_loss(h, yt)
    acc = O.accuracy(h, yt)
    loss.backward()
    out = float(loss.data()[0]), round(acc * len(y)), [(w.grad(), b.grad()) for w, b in params]
    O.Tape.reset()
    return out


def _net3(rng, inf, h1, h2, c):
    dims = [(h1, inf), (h2, h1), (c, h2)]
    return [(rng.uniform(-1, 1, d).astype(np.float32) * np.float32(np.sqrt(2.0 / d[1])), rng.uniform(-0.1, 0.1, d[0]).astype(np.float32)) for d in dims]


def _clear_of_relu_kinks(x, net, margin=2e-6):
    """Nudges the hidden layers' biases until no pre-activation of the batch lies within `margin` (relative to the layer's largest) of zero.
    A pre-activation within rounding of zero takes another sign under another summation order, and the ReLU mask it feeds flips: a
    discontinuity of the function, not an error of either side -- one flipped element of the second hidden layer moves EVERY row of dW1 by
    ~|dZ2| |W2| / B, i.e. by 1e-3 of that tensor's scale at batch 4096 (seen under the measurement forms).  The parity cases therefore run
    on data that stay clear of the kinks in float64; fp32 sums differ from those by ~1e-7 relative, far inside the margin."""
    h = x.astype(np.float64)
    out = []
    for l, (w, b) in enumerate(net):
        b = b.copy()
        if l < len(net) - 1:
            z = h @ w.astype(np.float64).T
            scale = float(np.abs(z).max()) + 1.0
            for j in range(w.shape[0]):
                for k in range(200):
                    if np.abs(z[:, j] + np.float64(b[j])).min() > margin * scale:
                        break
                    b[j] = np.float32(b[j] + (k + 1) * 3e-4 * (1 if k % 2 == 0 else -1))
                else:
                    raise AssertionError(f"layer {l + 1} unit {j}: no bias within reach keeps the batch clear of the ReLU kink")
            h = np.maximum(z + b.astype(np.float64), 0.0)
        out.append((w, b))
    return out


def _call_deep(ctx, src, batch, inf, net_dev, fuses=None, tick=None, log=None):
    from taper_amd import hip
    layers = (hip.Mlp3Layer * 3)()
    grads = []
    for l, (dw_, db_, w, b) in enumerate(net_dev):
        gw, gb = ctx.empty(w.size), ctx.empty(b.size)
        grads.append((gw, gb))
        wf = C.cast(C.pointer(fuses[l][0]), C.c_void_p) if fuses else None
        bf = C.cast(C.pointer(fuses[l][1]), C.c_void_p) if fuses else None
        layers[l] = hip.Mlp3Layer(int(dw_), int(db_), int(gw), int(gb), wf, bf, w.shape[0])
    loss, nc = ctx.empty(1), ctx.empty(1)
    metrics, cap, state, adv = log if log else (None, 0, None, 0)
    ctx.call("th_mlp2_xent_deep", C.byref(src), batch, inf, C.cast(layers, C.c_void_p), loss, nc, metrics, cap, state, adv, tick)
    return dict(loss=loss, nc=nc, grads=grads)


DEEP = [(1024, 784, 128, 64, 10), (4096, 784, 128, 64, 10), (16384, 784, 128, 64, 10), (256, 784, 128, 64, 10), (1000, 100, 64, 32, 5),
        (40, 36, 32, 16, 16), (5000, 784, 96, 48, 10), (2048, 64, 128, 128, 3), (12288 + 5, 784, 128, 64, 10),
        (1024, 784, 100, 52, 10), (600, 100, 36, 20, 5), (4100, 784, 116, 12, 10), (13000, 784, 100, 52, 10)]     # (ragged tiles in both hidden layers: r05)


@pytest.mark.parametrize("batch,inf,h1,h2,c", DEEP)
def test_mlp2_deep_dense_rows(ctx, O, batch, inf, h1, h2, c):
    """th_mlp2_xent_deep against the oracle's unfused chain: loss, hit count (exact), all six gradients; two calls give the same bits"""
    from taper_amd._lib import hip as lib
    assert lib.th_mlp2_xent_deep_supported(batch, inf, h1, h2, c, batch) == 1
    rng = np.random.default_rng(batch + inf + h1 + h2 + c)
    x = (rng.integers(0, 256, (batch, inf)) * (rng.uniform(0, 1, (batch, inf)) < 0.3)).astype(np.float32) / np.float32(255.0)
    y = rng.integers(0, c, batch).astype(np.float32)
    net = _clear_of_relu_kinks(x, _net3(rng, inf, h1, h2, c))
    ref_loss, ref_hits, ref_grads = _oracle3(O, x, y, net)
    net_dev = [(ctx.upload(w), ctx.upload(b), w, b) for w, b in net]
    dx, dy = ctx.upload(x), ctx.upload(y)
    src = RowSource(int(dx), int(dy), None, None, 0, batch)
    out = _call_deep(ctx, src, batch, inf, net_dev)
    assert ctx.download(out["loss"], 1)[0] == pytest.approx(ref_loss, rel=RTOL, abs=1e-6)
    assert ctx.download(out["nc"], 1)[0] == ref_hits                          # index work: exact
    for l, ((gw, gb), (rw, rb), (w, b)) in enumerate(zip(out["grads"], ref_grads, net)):
        got_w, got_b = ctx.download(gw, w.shape), ctx.download(gb, b.shape)
        close(got_w, np.asarray(rw).reshape(w.shape), atol=1e-6)
        close(got_b, np.asarray(rb).reshape(b.shape), atol=1e-6)
        margins.check(f"dw{l + 1}", got_w, np.asarray(rw).reshape(w.shape), 1e-4, test="test_mlp2_deep_dense_rows")
        margins.check(f"db{l + 1}", got_b, np.asarray(rb).reshape(b.shape), 1e-4, test="test_mlp2_deep_dense_rows")
    out2 = _call_deep(ctx, src, batch, inf, net_dev)
    for (gw, gb), (gw2, gb2), (w, b) in zip(out["grads"], out2["grads"], net):
        np.testing.assert_array_equal(ctx.download(gw, w.size), ctx.download(gw2, w.size))
        np.testing.assert_array_equal(ctx.download(gb, b.size), ctx.download(gb2, b.size))
    np.testing.assert_array_equal(ctx.download(out["loss"], 1), ctx.download(out2["loss"], 1))
    for (dw_, db_, w, b) in net_dev:                                            # parameters are only read without a fuse
        np.testing.assert_array_equal(ctx.download(dw_, w.shape), w)


def test_mlp2_deep_rows_through_the_index_vector_with_adam(ctx, O):
    """the reference's model on rows idx[(cursor + r) % n] of a resident set, wrapping at the epoch's end, with Adam for all six parameters
    in the finish launch at the t the rows launch opened, and the step log"""
    n_rows, batch, cursor, inf, h1, h2, c = 5000, 2048, 4000, 784, 128, 64, 10
    rng = np.random.default_rng(77)
    data = (rng.integers(0, 256, (n_rows, inf)) * (rng.uniform(0, 1, (n_rows, inf)) < 0.25)).astype(np.float32) / np.float32(255.0)
    labels = rng.integers(0, c, n_rows).astype(np.float32)
    idx = rng.permutation(n_rows).astype(np.int32)
    rows = idx[(cursor + np.arange(batch)) % n_rows]
    net = _clear_of_relu_kinks(data[rows], _net3(rng, inf, h1, h2, c))
    ref_loss, ref_hits, ref_grads = _oracle3(O, data[rows], labels[rows], net)
    lr, t = 1e-3, 6
    net_dev = [(ctx.upload(w), ctx.upload(b), w, b) for w, b in net]
    tick, dlr = ctx.upload(np.array([t, 0], np.int32)), ctx.upload(np.array([lr], np.float32))
    moms, fuses = [], []
    for (dw_, db_, w, b) in net_dev:
        ent = []
        for p, a in ((dw_, w), (db_, b)):
            m, v = ctx.zeros(a.size), ctx.zeros(a.size)
            moms.append((p, m, v, a))
            ent.append(AdamFuse(int(p), int(m), int(v), int(tick), int(dlr), 0.9, 0.999, 1e-8, 1e-4))
        fuses.append(ent)
    dd, dl, di = ctx.upload(data), ctx.upload(labels), ctx.upload(idx)
    state = ctx.upload(np.array([3, cursor], np.int64))
    src = RowSource(int(dd), int(dl), int(di), state.offset(8), n_rows, n_rows)
    metrics = ctx.zeros(2 * 8)
    out = _call_deep(ctx, src, batch, inf, net_dev, fuses=fuses, tick=tick, log=(metrics, 8, state, batch))
    assert ctx.download(tick, 2, np.int32)[0] == t + 1
    assert ctx.download(out["loss"], 1)[0] == pytest.approx(ref_loss, rel=RTOL, abs=1e-6)
    assert ctx.download(out["nc"], 1)[0] == ref_hits
    np.testing.assert_array_equal(ctx.download(state, 2, np.int64), [4, cursor + batch])
    m = ctx.download(metrics, 16)
    assert m[6] == ctx.download(out["loss"], 1)[0] and m[7] == ref_hits
    flat_ref = [g for pair in ref_grads for g in pair]
    for k, ((p, m_, v_, a), g) in enumerate(zip(moms, flat_ref)):
        p_ref, m_ref, v_ref = _adam_ref(O, a.reshape(-1), np.asarray(g, np.float32).reshape(-1), lr, t + 1)
        margins.check(f"param{k}_m", ctx.download(m_, a.size), m_ref, 1e-4, test="test_mlp2_deep_rows_through_the_index_vector_with_adam")
        margins.check_adam_weights(f"param{k}_after_adam", ctx.download(p, a.size), p_ref, v_ref, lr, 1, 2e-2, test="test_mlp2_deep_rows_through_the_index_vector_with_adam")


def test_mlp2_deep_limits_are_errors(ctx):
    from taper_amd._lib import TaperError, hip as lib
    assert lib.th_mlp2_xent_deep_supported(1024, 784, 128, 70, 10, 60000) == 0     # the hidden sizes: multiples of 4
    assert lib.th_mlp2_xent_deep_supported(1024, 784, 102, 64, 10, 60000) == 0
    assert lib.th_mlp2_xent_deep_supported(1024, 784, 100, 72, 10, 60000) == 1
    assert lib.th_mlp2_xent_deep_supported(1024, 784, 128, 144, 10, 60000) == 0
    assert lib.th_mlp2_xent_deep_supported(1024, 784, 128, 64, 10, 60000) == 1


def test_trainer_falls_back_when_the_large_batch_step_cannot_take_the_parameters():
    """the large-batch route is chosen on the FULL predicate (shapes AND the parameters' state).  A gradient left on W1 by the
    caller (the step writes gradients, it never accumulates) sends the epoch through the gathered launch-per-layer forms -- which do
    accumulate, like the reference (ops.rs:124-151) -- instead of failing inside the step; the next epoch (every step ended with
    zero_grad) takes th_mlp2_xent again.  Both epochs against the oracle's loop, which starts from the same left-over gradient."""
    import taper_amd as T
    from tests import backends
    H, Orc = backends.get("hip"), backends.get("oracle")
    Orc.set_zero_sentinel(True)
    rng = np.random.default_rng(31)
    spec = backends.nonzero_biases(backends.mlp_baseline(rng), rng)
    n, batch, lr = 2048, 1024, 1e-3
    x, y = backends.mnist_like(rng, n)
    hm, om = H.sequential(spec), Orc.sequential(spec)
    hopt, oopt = T.Adam(hm.parameters(), lr, None, None, 1e-4), Orc.m.Adam(om.parameters(), lr, None, None, 1e-4)
    left = (rng.standard_normal(hm.parameters()[0].shape()) * 1e-3).astype(np.float32)
    hm.parameters()[0].set_grad(left)
    om.parameters()[0].set_grad(left)
    tr = T.Trainer(hm, hopt)
    loader = T.DataLoader(T.MNISTDataset.from_host(x, y), batch, False)
    calls = []
    for epoch in range(2):
        before = _mlp2_calls()
        # (the first epoch eagerly: its first step accumulates onto the left-over gradient through the unfused forms and Adam::step, the
        # later ones take the fused forms -- a change of step form a captured epoch cannot follow; the second epoch is captured)
        ep = tr.run_epoch(loader, T.Trainer.EAGER if epoch == 0 else T.Trainer.GRAPH)
        calls.append(_mlp2_calls() - before)
        ref = [om.train_step(oopt, x[s * batch:(s + 1) * batch], y[s * batch:(s + 1) * batch], (batch, 784)) for s in range(n // batch)]
        margins.check(f"losses_epoch{epoch}", ep["losses"], [r["loss"] for r in ref], 1e-5)
    assert calls[0] == 0 and calls[1] >= 1, calls
    T.Tape.reset()
