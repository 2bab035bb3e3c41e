"""The step log (csrc/step_log_dev.h) through every C-ABI entry that writes it, on raw buffers: th_log_step, th_softmax_xent_fwd (its
one-workgroup and its multi-workgroup form), th_linear_xent_head_masked (the in-kernel log and head_finish_kernel), th_linear_xent_wide_ex,
th_wide_head_grads, th_mlp3_xent, th_conv_chain_mlp3_xent, th_mlp2_xent and th_mlp2_xent_deep -- what tests/test_gpu_step_tails.py asks
of th_mlp_tail, asked of all of them.  Each row runs at the smallest shape the entry takes: the kernels can go wrong on the state words,
not on the shape.  (The three-launch and the chain rows take the smallest shapes that tests/test_gpu_mlp2.py and
tests/test_gpu_chain_mlp3.py already hold to the oracle -- 33 x 36-32-16, 40 x 36-32-16-16, 16 images with 3 classes -- not the corner of
their *_supported queries, which no parity test has run.)  Every row is crossed with that file's LOG_STATES: below, at and above the
capacity, capacity 3, beyond 2^32 with a 32-bit capacity and with a capacity above 2^32.

Every case, exactly: slot state0 mod capacity holds the two floats the same launch wrote to d_loss[0] and d_ncorrect[0]; every other slot
of a pattern-filled metrics buffer keeps its fill; state == [state0 + 1, state1 + advance]; loss, hit count and every gradient the entry
writes equal, as uint32, those of the same launch with (capacity, state0) = (4096, 5) -- the log influences nothing else.  The sites that
stay written out (log_step_kernel, mlp2_finish_kernel: DESIGN.md section 3) are held to the shared definition by the same rows.

The data-parallel entries (th_mlp_tail_dp, th_wide_head_grads_dp) need two processes: they reach the same kernels' log through the same
launch functions and keep their coverage in tests/test_gpu_dp_inkernel.py.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_chain import REFERENCE, _images, _params
from tests.test_gpu_step_tails import LOG_STATES

pytestmark = pytest.mark.gpu
STATE1 = (1 << 35) + 11


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


def _down(ctx, bufs):
    return {k: ctx.download(b, (n,)) for k, (b, n) in bufs.items()}


def _layers(ctx, rng, dims, outs):
    """th_mlp3_layer records of Linear layers (out, in) with fresh gradient buffers, which join `outs`"""
    from taper_amd import hip
    layers, keep = (hip.Mlp3Layer * 3)(), []
    for l, (o, i) in enumerate(dims):
        w = ctx.upload((rng.uniform(-1, 1, (o, i)) * np.sqrt(2.0 / i)).astype(np.float32))
        b = ctx.upload(rng.uniform(-0.1, 0.1, o).astype(np.float32))
        outs[f"dw{l}"], outs[f"db{l}"] = (ctx.empty(o * i), o * i), (ctx.empty(o), o)
        layers[l] = hip.Mlp3Layer(int(w), int(b), int(outs[f"dw{l}"][0]), int(outs[f"db{l}"][0]), None, None, o)
        keep += [w, b]
    return layers, keep


# ---- one function per row: run(ctx, metrics, capacity, state, advance) -> every array the launch wrote (loss and nc among them) ----

def run_log_step(ctx, *log):
    loss, nc = ctx.upload(np.array([0.625], np.float32)), ctx.upload(np.array([3.0], np.float32))
    ctx.call("th_log_step", loss, nc, *log)
    return _down(ctx, dict(loss=(loss, 1), nc=(nc, 1)))


def _xent(batch):
    def run(ctx, *log):
        classes = 2
        rng = np.random.default_rng(batch)
        logits = ctx.upload(rng.standard_normal((batch, classes)).astype(np.float32))
        y = ctx.upload(rng.integers(0, classes, batch).astype(np.float32))
        n = batch * classes
        o = dict(logp=(ctx.empty(n), n), loss=(ctx.empty(1), 1), argmax=(ctx.empty(batch), batch), nc=(ctx.empty(1), 1), dunit=(ctx.empty(n), n))
        ctx.call("th_softmax_xent_fwd", logits, y, batch, classes, o["logp"][0], o["loss"][0], o["argmax"][0], o["nc"][0], o["dunit"][0], *log, None)
        return _down(ctx, o)
    return run


def _head(batch):
    def run(ctx, *log):
        k, c = 4, 2
        rng = np.random.default_rng(batch)
        h = ctx.upload(np.maximum(rng.standard_normal((batch, k)), 0).astype(np.float32))
        w, b = ctx.upload(rng.uniform(-0.3, 0.3, (c, k)).astype(np.float32)), ctx.upload(rng.uniform(-0.1, 0.1, c).astype(np.float32))
        y = ctx.upload(rng.integers(0, c, batch).astype(np.float32))
        o = dict(logits=(ctx.empty(batch * c), batch * c), loss=(ctx.empty(1), 1), nc=(ctx.empty(1), 1), dh=(ctx.empty(batch * k), batch * k),
                 dw=(ctx.empty(c * k), c * k), db=(ctx.empty(c), c))
        ctx.call("th_linear_xent_head_masked", h, w, b, y, batch, k, c, o["logits"][0], o["loss"][0], o["nc"][0], o["dh"][0], o["dw"][0], o["db"][0],
                 *log, None, None, None, 1)
        return _down(ctx, o)
    return run


def run_wide(ctx, *log):
    batch, k, c = 1, 33, 2
    rng = np.random.default_rng(33)
    h = ctx.upload(np.maximum(rng.standard_normal((batch, k)), 0).astype(np.float32))
    w, b = ctx.upload((rng.uniform(-1, 1, (c, k)) * np.sqrt(2.0 / k)).astype(np.float32)), ctx.upload(rng.uniform(-0.1, 0.1, c).astype(np.float32))
    y = ctx.upload(rng.integers(0, c, batch).astype(np.float32))
    o = dict(loss=(ctx.empty(1), 1), nc=(ctx.empty(1), 1), dx=(ctx.empty(batch * k), batch * k), dw=(ctx.empty(c * k), c * k), db=(ctx.empty(c), c),
             colsum=(ctx.empty(k), k))
    ctx.call("th_linear_xent_wide_ex", h, w, b, y, batch, k, c, o["loss"][0], o["nc"][0], o["dx"][0], o["dw"][0], o["db"][0], *log, None, o["colsum"][0])
    return _down(ctx, o)


def run_wide_grads(ctx, *log):
    n, k, classes, conv_c = 1, 16, 1, 4
    rng = np.random.default_rng(16)
    x = ctx.upload(rng.standard_normal((n, k)).astype(np.float32))
    dl = np.zeros((n, 16), np.float32)
    dl[:, :classes] = rng.standard_normal((n, classes)).astype(np.float32)
    rs = ctx.upload(np.array([[1.25, 1.0]], np.float32))
    cbp = ctx.upload(rng.standard_normal((n, conv_c)).astype(np.float32))
    o = dict(dw=(ctx.empty(classes * k), classes * k), db=(ctx.empty(classes), classes), gcb=(ctx.empty(conv_c), conv_c), loss=(ctx.empty(1), 1),
             nc=(ctx.empty(1), 1))
    ctx.call("th_wide_head_grads", x, ctx.upload(dl), rs, cbp, n, k, classes, conv_c, o["dw"][0], o["db"][0], o["gcb"][0], o["loss"][0], o["nc"][0],
             *log, None, None, None)
    return _down(ctx, o)


def run_mlp3(ctx, *log):
    B, in_f, h1, h2, c = 16, 16, 16, 16, 1
    rng = np.random.default_rng(3)
    x, y = ctx.upload(rng.uniform(0, 1, (B, in_f)).astype(np.float32)), ctx.upload(np.zeros(B, np.float32))
    o = dict(dx=(ctx.empty(B * in_f), B * in_f), loss=(ctx.empty(1), 1), nc=(ctx.empty(1), 1))
    layers, keep = _layers(ctx, rng, [(h1, in_f), (h2, h1), (c, h2)], o)
    ctx.call("th_mlp3_xent", x, y, B, in_f, C.cast(layers, C.c_void_p), o["dx"][0], o["loss"][0], o["nc"][0], *log, None, None)
    return _down(ctx, o)


def run_chain_mlp3(ctx, *log):
    from taper_amd import hip
    n, c = 16, 3
    rng = np.random.default_rng(9)
    cbufs = [(ctx.upload(w), ctx.upload(b)) for w, b in _params(REFERENCE, 5)]
    stages, ns = hip.conv_stages([(dw, db, c_out, post) for (dw, db), (_, c_out, post) in zip(cbufs, REFERENCE)])
    x, y = ctx.upload(_images(n, 7)), ctx.upload(rng.integers(0, c, n).astype(np.float32))
    o = dict(means=(ctx.empty(n * 128), n * 128), cnt=(ctx.empty(n * 128), n * 128), dx=(ctx.empty(n * 128), n * 128), gb=(ctx.empty(128), 128),
             loss=(ctx.empty(1), 1), nc=(ctx.empty(1), 1))
    layers, keep = _layers(ctx, rng, [(128, 128), (64, 128), (c, 64)], o)
    gap = hip.Mlp3Gap(int(o["cnt"][0]), int(o["gb"][0]), 49, None)
    ctx.call("th_conv_chain_mlp3_xent", x, C.cast(stages, C.c_void_p), ns, o["means"][0], o["cnt"][0], n, 1, 28, 28, y, C.cast(layers, C.c_void_p),
             o["dx"][0], o["loss"][0], o["nc"][0], *log, None, C.cast(C.pointer(gap), C.c_void_p))
    return _down(ctx, o)


def _mlp2(deep):
    def run(ctx, *log):
        from taper_amd.hip import RowSource
        batch, inf, h1, h2, c = (40, 36, 32, 16, 16) if deep else (33, 36, 32, 0, 16)
        rng = np.random.default_rng(2 + deep)
        rows, labels = ctx.upload(rng.uniform(0, 1, (batch, inf)).astype(np.float32)), ctx.upload(rng.integers(0, c, batch).astype(np.float32))
        src = RowSource(int(rows), int(labels), None, None, 0, batch)
        o = dict(loss=(ctx.empty(1), 1), nc=(ctx.empty(1), 1))
        dims = [(h1, inf), (h2, h1), (c, h2)] if deep else [(h1, inf), (c, h1)]
        layers, keep = _layers(ctx, rng, dims, o)
        if deep:
            ctx.call("th_mlp2_xent_deep", C.byref(src), batch, inf, C.cast(layers, C.c_void_p), o["loss"][0], o["nc"][0], *log, None)
        else:
            L = layers
            ctx.call("th_mlp2_xent", C.byref(src), batch, inf, h1, c, L[0].d_w, L[0].d_b, L[1].d_w, L[1].d_b, L[0].d_dw, L[0].d_db, L[1].d_dw,
                     L[1].d_db, o["loss"][0], o["nc"][0], *log, None, None, None, None, None)
        return _down(ctx, o)
    return run


# the smallest batch that reaches each form: th_softmax_xent_fwd runs as one workgroup up to 1024 rows; th_linear_xent_head logs in the
# kernel up to 64 rows (16: a quarter chunk) and in head_finish_kernel above
ROWS = {
    "log_step": (run_log_step, 64), "xent_one_wg": (_xent(1), 1), "xent_rows_finish": (_xent(1025), 1025), "head_in_kernel": (_head(16), 16),
    "head_finish": (_head(65), 65), "wide_ex": (run_wide, 1), "wide_head_grads": (run_wide_grads, 1), "mlp3": (run_mlp3, 16),
    "chain_mlp3": (run_chain_mlp3, 16), "mlp2": (_mlp2(False), 33), "mlp2_deep": (_mlp2(True), 40),
}
_ref_cache = {}


def _fill(slots):
    return (np.arange(2 * slots, dtype=np.uint32) + np.uint32(0x3F000000)).reshape(slots, 2)   # distinct finite floats near 0.5


def run_logged(ctx, row, capacity, state0):
    """-> (what the launch wrote, the metrics buffer as uint32, the state words)"""
    run, advance = ROWS[row]
    slots = min(capacity, 4096)
    metrics = ctx.upload(_fill(slots))
    state = ctx.upload(np.array([state0, STATE1], np.int64))
    out = run(ctx, metrics, capacity, state, advance)
    return out, ctx.download(metrics, (slots, 2), np.uint32), ctx.download(state, (2,), np.int64)


def reference(ctx, row):
    if row not in _ref_cache:
        _ref_cache[row] = run_logged(ctx, row, 4096, 5)[0]
    return _ref_cache[row]


@pytest.mark.parametrize("capacity,state0", LOG_STATES)
@pytest.mark.parametrize("row", list(ROWS))
def test_step_log(ctx, row, capacity, state0):
    ref = reference(ctx, row)
    slot = state0 % capacity                     # Python integers
    slots = min(capacity, 4096)
    assert slot < slots                          # (LOG_STATES is chosen so: the test's buffer holds the slot)
    out, metrics, state = run_logged(ctx, row, capacity, state0)
    want = _fill(slots)
    want[slot] = [out["loss"].view(np.uint32)[0], out["nc"].view(np.uint32)[0]]
    np.testing.assert_array_equal(metrics, want)
    assert state.tolist() == [state0 + 1, STATE1 + ROWS[row][1]]
    assert set(out) == set(ref)
    for k in ref:                                # loss, hit count, every gradient: the log influences none of them
        np.testing.assert_array_equal(out[k].view(np.uint32), ref[k].view(np.uint32), err_msg=k)
