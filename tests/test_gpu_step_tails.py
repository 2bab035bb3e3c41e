"""The odd workgroups of the MLP step's two launches, through the C ABI on raw buffers:

th_linear_fwd_ex's spare workgroup (adam_slices_then_tick: the carried Adam slices and the step counter) -- p / m / v
bit-identical to a stand-alone th_adam_slices launch on copies of the same buffers, t advanced by exactly one, H
bit-identical to th_linear_fwd, over every path of the role: slices shorter and longer than one stride of the
workgroup, ragged and unaligned ends, shared and per-slice counters and learning rates, no tick, the update guard;

th_mlp_tail's lead head workgroup (the step log): slot, state words, loss and hit count against the same integer
arithmetic in numpy, over the wrap branch, the 32-bit and the 64-bit remainder; the capacity influences nothing else.
"""
import ctypes as C

import numpy as np
import pytest

from taper_amd.hip import AdamFuse, AdamSlice

pytestmark = pytest.mark.gpu
MAX_SLICES = 4   # TH_MAX_ADAM_SLICES
BETAS = (0.9, 0.999, 1e-8, 1e-4)


@pytest.fixture(scope="module")
def ctx():
    from taper_amd import hip
    c = hip.Ctx(0)
    yield c
    c.close()


# ---- th_linear_fwd_ex ---------------------------------------------------------------------------------------------------------

# (batch, in, hidden, threads of the launch): one tile on the 4-wave instance; the MNIST layer on the 16-wave instance with the XCD map
FWD_SHAPES = {"nw4": (16, 32, 16, 256), "nw16": (64, 784, 128, 1024)}
_fwd_cache = {}


def fwd_operands(ctx, key):
    """x, w, b on the device and H = th_linear_fwd of them, computed once per shape"""
    if key not in _fwd_cache:
        batch, inf, hid, _ = FWD_SHAPES[key]
        rng = np.random.default_rng(batch + inf)
        x = ctx.upload(rng.uniform(0, 1, (batch, inf)).astype(np.float32))
        w = ctx.upload(rng.uniform(-0.1, 0.1, (hid, inf)).astype(np.float32))
        b = ctx.upload(rng.uniform(-0.1, 0.1, hid).astype(np.float32))
        h = ctx.empty(batch * hid)
        ctx.call("th_linear_fwd", x, w, b, h, batch, inf, hid, 1)
        _fwd_cache[key] = (x, w, b, ctx.download(h, (batch, hid)))
    return _fwd_cache[key]


def slice_specs(case, threads):
    """[(n, p misaligned by 4 bytes, own t / lr buffers)]"""
    return {
        "none": [],
        "one": [(10, False, False)],
        "two": [(1280, False, False), (10, False, False)],                              # the step's W2, b2
        "max_ragged": [(1280, False, False), (10, False, False), (1281, False, False), (7, False, False)],
        "general": [(4 * threads + 4, False, False), (10, False, False)],               # longer than one quad per thread
        "misaligned": [(1280, True, False), (1281, True, False)],                       # scalar path, whole and ragged
        "own_t": [(1280, False, False), (10, False, True)],                             # per-slice step size
    }[case]


class Slices:
    """device buffers of some carried slices, twice: one set for the launch under test, one for the stand-alone reference"""

    def __init__(self, ctx, specs, t, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.specs = ctx, specs
        self.t0 = [t] + [t + 3 for _ in specs]                 # [0] the shared counter, [1 + i] slice i's own
        self.sets = []
        host = []
        for n, _, _ in specs:
            host.append([rng.uniform(-0.1, 0.1, n + 1).astype(np.float32), (rng.standard_normal(n + 1) * 0.01).astype(np.float32),
                         rng.uniform(0, 1e-4, n + 1).astype(np.float32), (rng.standard_normal(n + 1) * 0.01).astype(np.float32)])
        for _ in range(2):
            ticks = ctx.upload(np.array(self.t0 + [0], np.int32))
            lrs = ctx.upload(np.array([1e-3] + [3e-3 + 1e-3 * i for i in range(len(specs))], np.float32))
            bufs = [[ctx.upload(a) for a in h] for h in host]
            arr = (AdamSlice * MAX_SLICES)()
            for i, ((n, mis, own), (p, m, v, g)) in enumerate(zip(specs, bufs)):
                off = 4 if mis else 0
                ti, li = (4 * (1 + i), 4 * (1 + i)) if own else (0, 0)
                arr[i] = AdamSlice(int(g), n, AdamFuse(int(p) + off, int(m) + off, int(v) + off, int(ticks) + ti, int(lrs) + li, *BETAS))
            self.sets.append(dict(ticks=ticks, lrs=lrs, bufs=bufs, arr=arr))
        self.host = host

    def state(self, which):
        s = self.sets[which]
        return [[self.ctx.download(b, (n + 1,)) for b in bufs[:3]] for bufs, (n, _, _) in zip(s["bufs"], self.specs)]

    def ticks(self, which):
        return self.ctx.download(self.sets[which]["ticks"], (len(self.t0) + 1,), np.int32)


def run_fwd_ex(ctx, key, sl, with_tick=True):
    batch, inf, hid, _ = FWD_SHAPES[key]
    x, w, b, h_ref = fwd_operands(ctx, key)
    h = ctx.empty(batch * hid)
    s = sl.sets[0]
    ctx.call("th_linear_fwd_ex", x, w, b, h, batch, inf, hid, 1, s["arr"] if sl.specs else None, len(sl.specs), s["ticks"] if with_tick else None)
    np.testing.assert_array_equal(ctx.download(h, (batch, hid)).view(np.uint32), h_ref.view(np.uint32))


def assert_same_bits(got, want):
    for i, (gs, ws) in enumerate(zip(got, want)):
        for name, g, w in zip("pmv", gs, ws):
            np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=f"slice {i} {name}")


@pytest.mark.parametrize("t", [1, 2, 1000, 4097])
@pytest.mark.parametrize("case", ["none", "one", "two", "max_ragged", "general", "misaligned", "own_t"])
@pytest.mark.parametrize("key", ["nw4", "nw16"])
def test_fwd_ex_slices_and_tick(ctx, key, case, t):
    specs = slice_specs(case, FWD_SHAPES[key][3])
    sl = Slices(ctx, specs, t, seed=len(specs) * 7 + t)
    run_fwd_ex(ctx, key, sl)
    if specs:
        ctx.call("th_adam_slices", sl.sets[1]["arr"], len(specs))          # the same updates, stand-alone, counters as they stood
    assert_same_bits(sl.state(0), sl.state(1))
    for (n, _, _), got, h in zip(specs, sl.state(0), sl.host):             # ... and they did update, up to the slice's end and no further
        assert not np.array_equal(got[0][:n], h[0][:n])
    want = np.array(sl.t0 + [0], np.int32)
    want[0] += 1                                                           # the shared counter opens the next step; nothing else moves
    np.testing.assert_array_equal(sl.ticks(0), want)
    np.testing.assert_array_equal(sl.ticks(1), np.array(sl.t0 + [0], np.int32))


@pytest.mark.parametrize("key", ["nw4", "nw16"])
def test_fwd_ex_no_tick(ctx, key):
    sl = Slices(ctx, slice_specs("two", FWD_SHAPES[key][3]), 5, seed=3)
    run_fwd_ex(ctx, key, sl, with_tick=False)
    ctx.call("th_adam_slices", sl.sets[1]["arr"], 2)
    assert_same_bits(sl.state(0), sl.state(1))
    np.testing.assert_array_equal(sl.ticks(0), np.array(sl.t0 + [0], np.int32))


@pytest.mark.parametrize("case", ["two", "general"])
@pytest.mark.parametrize("key", ["nw4", "nw16"])
def test_fwd_ex_update_guard(ctx, key, case):
    """a non-zero guard word: nothing is applied, nothing ticks (the product is still formed); a zero one: the step word advances with t"""
    words = ctx.upload(np.array([1, 41], np.uint32))        # [0] guard, [1] step word
    sl = Slices(ctx, slice_specs(case, FWD_SHAPES[key][3]), 9, seed=5)
    try:
        ctx.call("th_ctx_set_update_guard", words, int(words) + 4)
        run_fwd_ex(ctx, key, sl)
        for got, h in zip(sl.state(0), sl.host):
            for g, w in zip(got, h[:3]):
                np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
        np.testing.assert_array_equal(sl.ticks(0), np.array(sl.t0 + [0], np.int32))
        np.testing.assert_array_equal(ctx.download(words, (2,), np.uint32), [1, 41])
        words2 = ctx.upload(np.array([0, 41], np.uint32))
        ctx.call("th_ctx_set_update_guard", words2, int(words2) + 4)
        run_fwd_ex(ctx, key, sl)
        assert sl.ticks(0)[0] == sl.t0[0] + 1
        np.testing.assert_array_equal(ctx.download(words2, (2,), np.uint32), [0, 42])
    finally:
        ctx.call("th_ctx_set_update_guard", None, None)
    ctx.call("th_adam_slices", sl.sets[1]["arr"], len(sl.specs))
    assert_same_bits(sl.state(0), sl.state(1))


# ---- th_mlp_tail: the step log of the lead head workgroup -------------------------------------------------------------------------

HID, CLS = 32, 10
_tail_cache = {}


def tail_data(batch, inf):
    rng = np.random.default_rng(batch * 31 + inf)
    return dict(x=rng.uniform(0, 1, (batch, inf)).astype(np.float32), h=np.maximum(rng.standard_normal((batch, HID)), 0).astype(np.float32),
                w1=(rng.uniform(-1, 1, (HID, inf)) * np.sqrt(2.0 / inf)).astype(np.float32), b1=rng.uniform(-0.1, 0.1, HID).astype(np.float32),
                w2=rng.uniform(-0.3, 0.3, (CLS, HID)).astype(np.float32), b2=rng.uniform(-0.1, 0.1, CLS).astype(np.float32),
                y=rng.integers(0, CLS, batch).astype(np.float32))


def run_tail(ctx, d, batch, inf, capacity, state0, state1, advance, slots):
    """one th_mlp_tail launch (with the fused Adam of W1 / b1, t = 1000) on fresh buffers; everything it wrote"""
    up = {k: ctx.upload(v) for k, v in d.items()}
    n1 = HID * inf
    dw1, db1, dw2, db2, loss, nc = ctx.empty(n1), ctx.empty(HID), ctx.empty(CLS * HID), ctx.empty(CLS), ctx.empty(1), ctx.empty(1)
    mw, vw, mb, vb = ctx.zeros(n1), ctx.zeros(n1), ctx.zeros(HID), ctx.zeros(HID)
    tick, lr = ctx.upload(np.array([1000, 0], np.int32)), ctx.upload(np.array([1e-3], np.float32))
    wf = AdamFuse(int(up["w1"]), int(mw), int(vw), int(tick), int(lr), *BETAS)
    bf = AdamFuse(int(up["b1"]), int(mb), int(vb), int(tick), int(lr), *BETAS)
    metrics = ctx.upload(np.full((slots, 2), -1.0, np.float32))
    state = ctx.upload(np.array([state0, state1], np.int64))
    ctx.call("th_mlp_tail", up["x"], up["h"], up["w2"], up["b2"], up["y"], batch, inf, HID, CLS, loss, nc, dw1, db1, dw2, db2, None, None,
             metrics, capacity, state, advance, C.byref(wf), C.byref(bf))
    out = dict(dw1=ctx.download(dw1, (n1,)), db1=ctx.download(db1, (HID,)), dw2=ctx.download(dw2, (CLS * HID,)), db2=ctx.download(db2, (CLS,)),
               w1=ctx.download(up["w1"], (n1,)), b1=ctx.download(up["b1"], (HID,)), mw=ctx.download(mw, (n1,)), vw=ctx.download(vw, (n1,)),
               mb=ctx.download(mb, (HID,)), vb=ctx.download(vb, (HID,)), loss=ctx.download(loss, (1,)), nc=ctx.download(nc, (1,)))
    return out, ctx.download(metrics, (slots, 2)), ctx.download(state, (2,), np.int64)


def tail_reference(ctx, batch, inf):
    """the same launch with a capacity nothing wraps at, and the loss / hit count in numpy (float64)"""
    if (batch, inf) not in _tail_cache:
        d = tail_data(batch, inf)
        out, metrics, state = run_tail(ctx, d, batch, inf, 1 << 40, 5, 0, 1, 8)
        logits = d["h"].astype(np.float64) @ d["w2"].T.astype(np.float64) + d["b2"]
        z = logits - logits.max(1, keepdims=True)
        nll = -(z - np.log(np.exp(z).sum(1, keepdims=True)))[np.arange(batch), d["y"].astype(int)]
        assert out["loss"][0] == pytest.approx(nll.mean(), rel=1e-5)
        assert out["nc"][0] == float((logits.argmax(1) == d["y"].astype(int)).sum())
        assert state.tolist() == [6, 1] and metrics[5].tolist() == [out["loss"][0], out["nc"][0]]
        _tail_cache[(batch, inf)] = (d, out)
    return _tail_cache[(batch, inf)]


# (capacity, state0): below and above each capacity (the wrap branch, 32-bit remainder), and beyond 2^32 (the 64-bit remainder)
LOG_STATES = [(4096, 5), (4096, 5000), (4096, 4096), (3, 2), (3, 7), (3, 3), (4096, (1 << 32) + 5), (3, (1 << 32) + 5), ((1 << 33) + 1, (1 << 34) + 7)]


@pytest.mark.parametrize("capacity,state0", LOG_STATES)
@pytest.mark.parametrize("inf", [48, 40], ids=["whole_tiles", "edge_tiles"])   # mlp_tail_exact_kernel / mlp_tail_kernel
@pytest.mark.parametrize("batch", [16, 64])
def test_tail_step_log(ctx, batch, inf, capacity, state0):
    d, ref = tail_reference(ctx, batch, inf)
    state1, advance = (1 << 35) + 11, batch
    slot = state0 if state0 < capacity else state0 % capacity          # th_log_step
    slots = min(capacity, 4096)
    assert slot < slots    # (the cases are chosen so: the log buffer of the test holds the slot)
    out, metrics, state = run_tail(ctx, d, batch, inf, capacity, state0, state1, advance, slots)
    want = np.full((slots, 2), -1.0, np.float32)
    want[slot] = [ref["loss"][0], ref["nc"][0]]
    np.testing.assert_array_equal(metrics.view(np.uint32), want.view(np.uint32))
    assert state.tolist() == [state0 + 1, state1 + advance]
    for k in ref:          # loss, hit count, every gradient and the fused updates: the capacity influences none of them
        np.testing.assert_array_equal(out[k].view(np.uint32), ref[k].view(np.uint32), err_msg=k)


# ---- the step size against an independent restatement ---------------------------------------------------------------------------

def _powisf2(a, b):
    """compiler-rt __powisf2 in float32 (what f32::powi lowers to, optim.rs:87-88): ONE power, its own loop"""
    a, r = np.float32(a), np.float32(1)
    while True:
        if b & 1:
            r = np.float32(r * a)
        b //= 2
        if b == 0:
            return r
        a = np.float32(a * a)


def _adam_f32(p, m, v, g, t, lr, b1, b2, eps, wd):
    """optim.rs:87-110 in numpy float32, operation by operation in the kernels' order (every float32 operation of the kernels is
    correctly rounded -- IEEE division and square root, no contraction -- so the bits must agree)"""
    f = np.float32
    b1, b2, eps, wd, lr = f(b1), f(b2), f(eps), f(wd), f(lr)
    bc1, bc2 = f(f(1) - _powisf2(b1, t)), f(f(1) - _powisf2(b2, t))
    step = f(lr * f(np.sqrt(bc2) / bc1))
    gj = g + wd * p
    m2 = b1 * m + f(f(1) - b1) * gj
    v2 = b2 * v + (f(f(1) - b2) * gj) * gj
    p2 = p - (step * m2) / (np.sqrt(v2) + eps)
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9375)], ids=["default", "dyadic"])
@pytest.mark.parametrize("t", [1, 2, 7, 1000, 4097, 12345])
def test_step_size_bits_against_numpy(ctx, t, betas):
    """adam_step_size raises both betas in one loop; th_adam_slices' p / m / v must carry the bits of two separate __powisf2 powers
    (the launches above are compared with th_adam_slices, which shares that function: this is the check that does not)"""
    n, lr, eps, wd = 1281, 1e-3, 1e-8, 1e-4
    rng = np.random.default_rng(t)
    p = rng.uniform(-0.1, 0.1, n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = rng.uniform(0, 1e-4, n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    dp, dm, dv, dg = ctx.upload(p), ctx.upload(m), ctx.upload(v), ctx.upload(g)
    tick, dlr = ctx.upload(np.array([t, 0], np.int32)), ctx.upload(np.array([lr], np.float32))
    arr = (AdamSlice * MAX_SLICES)()
    arr[0] = AdamSlice(int(dg), n, AdamFuse(int(dp), int(dm), int(dv), int(tick), int(dlr), betas[0], betas[1], eps, wd))
    ctx.call("th_adam_slices", arr, 1)
    want = _adam_f32(p, m, v, g, t, lr, betas[0], betas[1], eps, wd)
    for name, buf, w in zip("pmv", (dp, dm, dv), want):
        np.testing.assert_array_equal(ctx.download(buf, (n,)).view(np.uint32), w.view(np.uint32), err_msg=name)
