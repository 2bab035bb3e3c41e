#!/usr/bin/env python
"""In-kernel stamps of the MLP step's first launch (th_linear_fwd_ex: sgemm_small16_tick at 784 -> 128): where a tile workgroup
spends its time.  Needs the profile build of the kernel library (`make -C taper_amd/csrc PROFILE=1`: the FWD_STAMP points of
small16_body in small16_dev.h and the entry reading of fwd_tick.hip, 100 MHz wall clock, lane 0 of wave 0 and of the last wave that owns a whole K chunk, every workgroup).
The step's two launches run back to back on the stream as in the Trainer's graph (tools/step_tails_probe.py's chain), so the
launch finds X unread and W1 just rewritten by the gradient launch's Adam epilogue; after every `--steps` steps the stamps of the
LAST forward launch are read.

  stamp 0  entry                              3  last MFMA retired
        1  all operand loads issued           4  behind the barrier
        2  operands of the first MFMA landed  5  the store has returned
        6  the kernel's true entry, read in front of any argument use (stamp 0, "entry" of the body, lies behind the kernel's
           choice of role and its tile numbers, in front of the operand addresses)

Per wave (w0 = wave 0, wl = the last whole-chunk wave), medians over the tile workgroups, then over the samples, us:
  issue  1 - 0      land  2 - 1      mfma  3 - 2      wait  3 - 1 (loads issued -> all of them consumed)
  sync   4 - 3      store 5 - 4      body  5 - 0      end   5 - the launch's earliest stamp 0
  args   0 - 6 (true entry -> the body starts forming operand addresses)      entry_issue  1 - 6 (true entry -> all operand loads requested:
  what the kernel-argument fetches cost shows here)
and the workgroup that ends last (block id, its end).  A beyond-L2 round trip is about 0.4 us (an HBM miss: 900 cycles).

  python tools/prof_fwd.py [--batch 64] [--subtiles 1] [--samples 200] [--json OUT] [--root TREE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=200)
ap.add_argument("--steps", type=int, default=8, help="steps enqueued per sample")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--subtiles", type=int, default=1, help="the context's sub-tile switch (0: the 16 x 16 launch)")
ap.add_argument("--t0", type=int, default=1000, help="the step counter before every sample")
ap.add_argument("--json", default=None)
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose taper_amd package (and built libraries) to load")
args = ap.parse_args()
sys.path.insert(0, args.root)

from taper_amd import hip  # noqa: E402
from taper_amd._lib import hip as lib  # noqa: E402

if not hasattr(lib, "th_debug_fwd_prof"):
    sys.exit("prof_fwd.py: the loaded libtaper_hip.so is not a profile build (make -C taper_amd/csrc PROFILE=1)")
lib.th_debug_fwd_prof.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
lib.th_debug_fwd_prof.restype = C.c_int

IN, HID, OUT, B = 784, 128, 10, args.batch
plan = (C.c_int * 8)()
assert lib.th_debug_linear_fwd_ex_plan(B, IN, HID, args.subtiles, plan) == 0 and plan[0] == 1
rm, rn, waves, cpw, gx, gy, xcd = plan[1:8]
n_tiles = gx * (gy - 1)
assert n_tiles <= 320, "the profile build stamps the first 320 workgroups"
ctx = hip.Ctx(0)
ctx.call("th_linear_fwd_ex_set_subtiles", args.subtiles)
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


def step():
    ctx.call("th_linear_fwd_ex", x, p1, int(p1) + 4 * HID * IN, h, B, IN, HID, 1, carried, 2, tick)
    ctx.call("th_mlp_tail", x, h, p2, int(p2) + 4 * OUT * HID, y, B, IN, HID, OUT, loss, nc, g1, int(g1) + 4 * HID * IN, g2,
             int(g2) + 4 * OUT * HID, None, None, metrics, 4096, state, 1, C.byref(w1f), C.byref(b1f))


SEGS = (("issue", 1, 0), ("land", 2, 1), ("mfma", 3, 2), ("wait", 3, 1), ("sync", 4, 3), ("store", 5, 4), ("body", 5, 0), ("args", 0, 6),
        ("entry_issue", 1, 6))
rows = []
buf = np.zeros((n_tiles, 2, 8), np.int64)   # (slots 0..6 are stamps, 7 is unused)
for it in range(args.samples + 10):
    lib.th_memcpy_h2d(ctx.h, int(tick), tick0.ctypes.data, tick0.nbytes)
    for _ in range(args.steps):
        step()
    if lib.th_debug_fwd_prof(ctx.h, buf.ctypes.data, n_tiles) != 0:
        sys.exit("th_debug_fwd_prof failed")
    if it < 10:
        continue
    s = buf.astype(np.float64) * 0.01          # us
    start = s[:, 0, 0].min()
    row = {}
    for wi, wn in ((0, "w0"), (1, "wl")):
        for name, hi, lo in SEGS:
            row[f"{wn}_{name}"] = np.median(s[:, wi, hi] - s[:, wi, lo])
        row[f"{wn}_end"] = np.median(s[:, wi, 5] - start)
    end = s[:, :, 5].max(axis=1) - start
    row.update(first_to_last_entry=s[:, 0, 0].max() - start, slowest_end=end.max(), slowest_block=float(end.argmax()),
               slowest_wait=(s[:, :, 3] - s[:, :, 1]).max())
    rows.append(row)
out = {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0] if k != "slowest_block"}
blocks = np.array([int(r["slowest_block"]) for r in rows])
out["slowest_block_mode"] = int(np.bincount(blocks).argmax())
out["slowest_block_mode_frac"] = round(float(np.mean(blocks == out["slowest_block_mode"])), 3)
out.update(samples=len(rows), batch=B, subtile=f"{rm}x{rn}", waves=waves, chunks_per_wave=cpw, tile_workgroups=n_tiles, xcd_blocks=xcd)
for k, v in out.items():
    print(f"{k:28s} {v}")
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(json.dumps(out, indent=1) + "\n")
