#!/usr/bin/env python
"""What the ONE odd workgroup of the MLP step's first launch costs (sgemm_small16_tick's spare workgroup: the carried
Adam slices of W2 / b2 and the step counter), measured in situ like bench.py's StepKernels: raw buffers through the
C ABI, the two launches of the step (K1 th_linear_fwd_ex, K2 th_mlp_tail) as 16-step graph chains, HIP events, all
graphs alive until the end.  K1 is called in three ways:

  1  as the step calls it        2 carried slices + tick
  2  n_slices = 0, with tick     the spare workgroup only ticks
  3  n_slices = 0, tick = NULL   the plain tile launch (the spare workgroup leaves at once)

(1) - (3) bounds what shortening the spare workgroup can gain, (2) - (3) is the tick's share.  The variants are
measured in turn, `--reps` times over; the spread of a variant over the repetitions is the noise the differences
have to clear.  The counter is put back to --t0 before every timed group, so every variant's K2 forms its step size
from the same t (that block's length grows with log2 t).

  python tools/step_tails_probe.py [--reps 5] [--json OUT] [--root TREE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--t0", type=int, default=1000, help="the step counter at the start of every timed group")
ap.add_argument("--json", default=None, help="also write the figures to this file")
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose taper_amd package (and built libraries) to load")
args = ap.parse_args()
sys.path.insert(0, args.root)

from taper_amd import hip  # noqa: E402

IN, HID, OUT, STEPS = 784, 128, 10, 16
B = args.batch
ctx = hip.Ctx(0)
rng = np.random.default_rng(0)
f = lambda *shape: ctx.upload(rng.uniform(-0.05, 0.05, shape).astype(np.float32))
x, y = ctx.upload(rng.uniform(0, 1, (B, IN)).astype(np.float32)), ctx.upload(rng.integers(0, OUT, B).astype(np.float32))
n1, n2 = HID * IN + HID, OUT * HID + OUT
p1, g1, m1, v1 = f(n1), ctx.zeros(n1), ctx.zeros(n1), ctx.zeros(n1)
p2, g2, m2, v2 = f(n2), ctx.zeros(n2), ctx.zeros(n2), ctx.zeros(n2)
h, loss, nc = ctx.empty(B * HID), ctx.empty(1), ctx.empty(1)
metrics, state = ctx.zeros(2 * 4096), ctx.upload(np.zeros(2, np.int64))
tick0 = np.array([args.t0, 0], np.int32)
tick, lr = ctx.upload(tick0), ctx.upload(np.array([1e-3], np.float32))
adam = lambda p, m, v, off: hip.AdamFuse(int(p) + 4 * off, int(m) + 4 * off, int(v) + 4 * off, int(tick), int(lr), 0.9, 0.999, 1e-8, 1e-4)
w1f, b1f = adam(p1, m1, v1, 0), adam(p1, m1, v1, HID * IN)
carried = (hip.AdamSlice * 2)(hip.AdamSlice(int(g2), OUT * HID, adam(p2, m2, v2, 0)),
                              hip.AdamSlice(int(g2) + 4 * OUT * HID, OUT, adam(p2, m2, v2, OUT * HID)))


def k1(n_slices, with_tick):
    ctx.call("th_linear_fwd_ex", x, p1, int(p1) + 4 * HID * IN, h, B, IN, HID, 1, carried if n_slices else None, n_slices,
             tick if with_tick else None)


def k2():
    ctx.call("th_mlp_tail", x, h, p2, int(p2) + 4 * OUT * HID, y, B, IN, HID, OUT, loss, nc, g1, int(g1) + 4 * HID * IN, g2,
             int(g2) + 4 * OUT * HID, None, None, metrics, 4096, state, 1, C.byref(w1f), C.byref(b1f))


def capture(n_slices, with_tick):
    ctx.graph_begin()
    try:
        for _ in range(STEPS):
            k1(n_slices, with_tick)
            k2()
    finally:
        g = ctx.graph_end()
    for _ in range(3):
        ctx.graph_launch(g)
    ctx.sync()
    return g


def replay_us(g, groups=10, inner=12):
    e0, e1 = hip.Event(), hip.Event()
    ms = 0.0
    for _ in range(groups):
        hip.hip.th_memcpy_h2d(ctx.h, int(tick), tick0.ctypes.data, tick0.nbytes)
        ctx.sync()
        ctx.record(e0)
        for _ in range(inner):
            ctx.graph_launch(g)
        ctx.record(e1)
        ms += hip.Ctx.elapsed_ms(e0, e1)
    return ms * 1e3 / (groups * inner * STEPS)


VARIANTS = [("1 slices+tick", 2, True), ("2 tick only", 0, True), ("3 plain tiles", 0, False)]
graphs = [capture(n, t) for _, n, t in VARIANTS]
for g in graphs:      # one untimed pass: clocks and caches settle
    replay_us(g, groups=2)
runs = {name: [] for name, _, _ in VARIANTS}
for _ in range(args.reps):
    for (name, _, _), g in zip(VARIANTS, graphs):
        runs[name].append(round(replay_us(g), 4))
med = {k: statistics.median(v) for k, v in runs.items()}
spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
out = dict(batch=B, t0=args.t0, us_per_step=runs, median=med, spread=spread,
           slices_and_tick_us=round(med["1 slices+tick"] - med["3 plain tiles"], 4),
           tick_us=round(med["2 tick only"] - med["3 plain tiles"], 4), noise_us=max(spread.values()))
for k, v in runs.items():
    print(f"{k:16s} median {med[k]:7.3f} us/step   spread {spread[k]:.3f}   runs {v}")
print(f"(1)-(3) = {out['slices_and_tick_us']:.3f} us   (2)-(3) = {out['tick_us']:.3f} us   noise (largest spread) = {out['noise_us']:.3f} us")
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(json.dumps(out, indent=1) + "\n")
for g in graphs:
    ctx.graph_destroy(g)
