#!/usr/bin/env python3
"""The launches that apply Adam in their epilogue, timed one by one (A/B of two builds of the library): th_linear_bwd_adam at the shapes of
test_linear_bwd_adam_epilogue, th_mlp_tail with both updates fused at batch 64, th_adam_step on the MNIST MLP's arena,
th_linear_xent_wide_fused at the simple CNN's head.  Each as a captured graph of 50 launches replayed back to back (device time, not the
host's enqueue rate), the median of five windows.  One JSON line: {name: us per launch}.

  python tools/adam_sites_time.py [TREE]      TREE: the root of the build to time (default: this one)"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else str(Path(__file__).resolve().parent.parent))
from taper_amd import hip  # noqa: E402
from taper_amd.hip import AdamFuse  # noqa: E402

ctx = hip.Ctx(0)
rng = np.random.default_rng(0)


def timed(fn, reps=300):
    """a captured graph of 50 launches replayed back to back (device time, not the host's enqueue rate); the median of 5 windows of
    `reps` replays"""
    ctx.graph_begin()
    for _ in range(50):
        fn()
    g = ctx.graph_end()
    for _ in range(10):
        ctx.graph_launch(g)
    ctx.sync()
    best = []
    for _ in range(5):
        e0, e1 = hip.Event(), hip.Event()
        ctx.record(e0)
        for _ in range(reps):
            ctx.graph_launch(g)
        ctx.record(e1)
        ctx.sync()
        best.append(hip.Ctx.elapsed_ms(e0, e1) * 1e3 / (reps * 50))
    return round(sorted(best)[len(best) // 2], 3)


tick, dlr = ctx.upload(np.array([7, 0, 0, 0], np.int32)), ctx.upload(np.array([1e-3], np.float32))
fz = lambda n, p=None: AdamFuse(int(p if p is not None else ctx.upload(rng.uniform(-0.1, 0.1, n).astype(np.float32))), int(ctx.zeros(n)), int(ctx.zeros(n)), int(tick), int(dlr), 0.9, 0.999, 1e-8, 1e-4)
keep, out = [], {}
for batch, inf, outf, with_dx in [(64, 784, 128, False), (64, 128, 64, True), (16, 40, 24, False), (4096, 784, 128, False), (3000, 256, 130, True),
                                  (1024, 784, 128, False), (600, 64, 48, True)]:
    x = ctx.upload(rng.uniform(0, 1, (batch, inf)).astype(np.float32))
    w = ctx.upload(rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32))
    dy = ctx.upload((rng.standard_normal((batch, outf)) * 0.01).astype(np.float32))
    ya = ctx.upload(np.maximum(rng.standard_normal((batch, outf)), 0).astype(np.float32))
    dw, db, dx = ctx.empty(outf * inf), ctx.empty(outf), (ctx.empty(batch * inf) if with_dx else None)
    pw = ctx.upload(rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32))
    wf, bf = fz(outf * inf, pw), fz(outf)
    keep += [x, w, dy, ya, dw, db, dx, pw, wf, bf]
    fn = lambda: ctx.call("th_linear_bwd_adam", x, pw if with_dx else w, dy, ya, dx, dw, db, batch, inf, outf, 0, C.byref(wf), C.byref(bf))
    out[f"linear_bwd_adam_{batch}x{inf}x{outf}{'_dx' if with_dx else ''}"] = timed(fn, 300 if batch <= 1024 else 60)

batch, inf, hid, c = 64, 784, 128, 10
x = ctx.upload(rng.uniform(0, 1, (batch, inf)).astype(np.float32))
h = ctx.upload(np.maximum(rng.standard_normal((batch, hid)), 0).astype(np.float32))
w2, b2 = ctx.upload(rng.uniform(-0.3, 0.3, (c, hid)).astype(np.float32)), ctx.upload(rng.uniform(-0.1, 0.1, c).astype(np.float32))
y = ctx.upload(rng.integers(0, c, batch).astype(np.float32))
dw1, db1, dw2, db2, loss = ctx.empty(hid * inf), ctx.empty(hid), ctx.empty(c * hid), ctx.empty(c), ctx.empty(1)
wf, bf = fz(hid * inf), fz(hid)
out["mlp_tail_b64_fused"] = timed(lambda: ctx.call("th_mlp_tail", x, h, w2, b2, y, batch, inf, hid, c, loss, None, dw1, db1, dw2, db2, None, None, None, 0,
                                                   None, 0, C.byref(wf), C.byref(bf)))
n = 101770 + 2    # 784-128-10, padded to whole quads
p, g, m, v = ctx.upload(rng.uniform(-0.1, 0.1, n).astype(np.float32)), ctx.upload((rng.standard_normal(n) * 0.01).astype(np.float32)), ctx.zeros(n), ctx.zeros(n)
offs, has = ctx.upload(np.zeros(1, np.int64)), ctx.upload(np.ones(1, np.int32))
out["adam_step_101772"] = timed(lambda: ctx.call("th_adam_step", p, g, m, v, offs, has, 1, n, tick, dlr, 0.9, 0.999, 1e-8, 1e-4, 1))
# th_linear_xent_wide_fused (wide_head_kernel: W, b and the conv bias updated in the head's own launches), the simple CNN's head at batch 256
from taper_amd.hip import WideFuse  # noqa: E402
batch, c_conv, hw, c = 256, 64, 49, 10
k = c_conv * hw
hx = ctx.upload(np.maximum(rng.standard_normal((batch, k)), 0).astype(np.float32))
yy = ctx.upload(rng.integers(0, c, batch).astype(np.float32))
pw_, pb_, pcb_ = (ctx.upload((rng.uniform(-1, 1, n_) * 0.02).astype(np.float32)) for n_ in (c * k, c, c_conv))
gcb, dw_, db_, cs_, ls_ = ctx.empty(c_conv), ctx.empty(c * k), ctx.empty(c), ctx.empty(k), ctx.empty(1)
wfz = WideFuse(fz(c * k, pw_), fz(c, pb_), fz(c_conv, pcb_), int(gcb), c_conv, hw)
out["linear_xent_wide_fused_b256"] = timed(lambda: ctx.call("th_linear_xent_wide_fused", hx, pw_, pb_, yy, batch, k, c, ls_, None, dw_, db_, None, 0, None, 0, tick,
                                                            cs_, C.byref(wfz)), 100)
print(json.dumps(out))
