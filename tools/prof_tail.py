#!/usr/bin/env python
"""In-kernel stamps of the MLP step's second launch (mlp_tail_split_kernel<8,2,false> at batch 64, or with `--split 0` the
320-thread mlp_tail_exact_kernel<8,2,false,4>): which workgroup ends last.  Needs the profile build of the kernel library
(`make -C taper_amd/csrc PROFILE=1`: the TAIL_STAMP points of mlp_tail.hip, 100 MHz wall clock, thread 0 of every workgroup).  The step's two launches run back to back on the
stream as in the Trainer's graph; after every `--steps` steps the stamps of the LAST tail launch are read.

Per role (lead head workgroup = block 0, plain head workgroups = blocks 1..7, dW1 workgroups = the rest):
  body   stamp 7 - stamp 0 of the workgroup
  end    stamp 7 - the earliest stamp 0 of the launch (when the workgroup is done, on the launch's own clock)
  step   stamp 2 - stamp 1 (the step-size block: what of it is NOT hidden under the loads shows up as body time)
  issue  stamp 1 - stamp 0 (roles, addresses and the issue of every load)
  wait   stamp 3 - stamp 2 (the load wait that is left behind the step-size block)
  math   stamp 5 - stamp 3 (logits, softmax, dH, the dW1 / dW2 products)
  sync   stamp 6 - stamp 5 (partial sums to LDS and the final barrier)
In the instances with a helper wave the lead's stamp 7 is the later of thread 0's and the helper's.

The launch's split form (mlp_tail_split_kernel, the default; `--split 0` asks the context for the 320-thread form and reports the columns
above) stamps TWO waves per workgroup: lane 0 of logit wave 0 and lane 0 of operand wave 4 (a table of its own).  Per role then
  lg_issue  logit wave: stamp 1 - 0 (roles, addresses, the last of its 11..15 loads requested)
  lg_image  logit wave: stamp 3 - 1 (its two k-slices of W2 arrive and go to LDS; barrier 0: the image is whole)
  lg_math   logit wave: stamp 4 - 3 (the image back from LDS, H's load wait, logits, softmax, dlogits parked in LDS)
  op_issue  operand wave: stamp 1 - 0 (the last of its loads requested)
  op_wait   operand wave: stamp 3 - 1 (barrier 0, then at barrier 1 for the logit waves)
  op_math   operand wave: stamp 5 - 3 (dlogits back from LDS, dH, the dW1 / dW2 products)
  op_sync   operand wave: stamp 6 - 5 (partial sums to LDS and barrier 2)
  op_behind operand wave: stamp 7 - 6 (wave-ordered sums, stores, fused Adam of tile 0; head role: dW2, db1)
  lg_sync   logit wave: stamp 6 - 4 (barrier 1, then at barrier 2 for the operand waves)
  lg_behind logit wave: stamp 2 - 6 (dW1 workgroups: wave-ordered sums, stores, fused Adam of tile 1; 0 where it finishes nothing)
  parked    logit wave's stamp 4 from the earlier stamp 0 of the two waves (entry -> dlogits parked)
  lg_args / op_args                    stamp 0 - the wave's true entry (a wall-clock read in front of any argument use): the argument fetch
  lg_entry_issued / op_entry_issued    stamp 1 - the true entry (entry -> the last of the wave's loads requested)
(lg_sync / lg_behind, and the four columns from the true entry, only from a build that stamps them.)
body / end are the workgroup's stamp 7 -- the latest of its logit wave's, its operand wave's and, in the lead, the helper's -- from the
earlier stamp 0 of the two waves.

The shape is fixed (784-128-10, batch 64: 8 head + 200 dW1 workgroups); the role split below and the profile build's 256-workgroup
stamp table hold for that launch only.

  python tools/prof_tail.py [--samples 200] [--split 1] [--json OUT] [--root TREE]
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
ap.add_argument("--t0", type=int, default=1000, help="the step counter before every sample")
ap.add_argument("--split", type=int, default=1, help="the context's split switch (0: the 320-thread form; ignored by a tree without the switch)")
ap.add_argument("--json", default=None)
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose taper_amd package (and built libraries) to load")
args = ap.parse_args()
sys.path.insert(0, args.root)

from taper_amd import hip  # noqa: E402
from taper_amd._lib import hip as lib  # noqa: E402

if not hasattr(lib, "th_debug_tail_prof_all"):
    sys.exit("prof_tail.py: the loaded libtaper_hip.so is not a profile build (make -C taper_amd/csrc PROFILE=1)")
lib.th_debug_tail_prof_all.argtypes = [C.c_void_p, C.c_void_p]
lib.th_debug_tail_prof_all.restype = C.c_int

IN, HID, OUT, B = 784, 128, 10, 64
N_HEAD, N_BLOCKS = 8, 208     # mlp_tail_launch: n_head = 8, n_dw = 8 * ceil(784 / 32) = 200
assert N_HEAD == (HID // 16 + 7) // 8 * 8 and N_BLOCKS - N_HEAD == (HID // 16 * -(-IN // 32) + 7) // 8 * 8 and N_BLOCKS <= 256
ctx = hip.Ctx(0)
SPLIT = bool(args.split) and hasattr(lib, "th_mlp_tail_set_split")
if hasattr(lib, "th_mlp_tail_set_split"):
    ctx.call("th_mlp_tail_set_split", int(SPLIT))
if SPLIT:
    lib.th_debug_tail_prof_op.argtypes = [C.c_void_p, C.c_void_p]
    lib.th_debug_tail_prof_op.restype = C.c_int
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


rows = []
buf, buf_op = np.zeros((256, 8), np.int64), np.zeros((256, 8), np.int64)


def split_row(s, o):
    """one sample of the split form: s = logit wave 0's stamps, o = operand wave 4's (us); s[:, 7] is the workgroup's end"""
    first = np.minimum(s[:, 0], o[:, 0])
    start = first.min()
    body, end = s[:, 7] - first, s[:, 7] - start
    dw = slice(N_HEAD, N_BLOCKS)
    row = {}
    cols = [("lg_issue", s, 1, 0), ("lg_image", s, 3, 1), ("lg_math", s, 4, 3), ("op_issue", o, 1, 0), ("op_wait", o, 3, 1), ("op_math", o, 5, 3),
            ("op_sync", o, 6, 5), ("op_behind", o, 7, 6)]
    if s[:, 6].any():   # a build whose logit waves work behind barrier 2
        own_end = np.maximum(s[:, 2], s[:, 6])   # (a logit wave that finishes nothing leaves no stamp 2 of this launch)
        s = s.copy()
        s[:, 2] = own_end
        cols += [("lg_sync", s, 6, 4), ("lg_behind", s, 2, 6)]
    if s[:, 5].any() and o[:, 2].any():   # a build that stamps the kernel's true entry (slot 5 of the logit wave's table, slot 2 of the operand wave's)
        cols += [("lg_args", s, 0, 5), ("lg_entry_issued", s, 1, 5), ("op_args", o, 0, 2), ("op_entry_issued", o, 1, 2)]
    for name, tab, hi, lo in cols:
        d = tab[:, hi] - tab[:, lo]
        row.update({f"lead_{name}": d[0], f"head_{name}": np.median(d[1:N_HEAD]), f"dw_{name}": np.median(d[dw])})
    parked = s[:, 4] - first
    row.update(lead_parked=parked[0], head_parked=np.median(parked[1:N_HEAD]), dw_parked=np.median(parked[dw]), last_block=float(end.argmax()))
    return dict(row, lead_body=body[0], lead_end=end[0], head_body=np.median(body[1:N_HEAD]), head_end=np.median(end[1:N_HEAD]),
                dw_body=np.median(body[dw]), dw_end=np.median(end[dw]), dw_end_max=end[dw].max(), launch=end.max(),
                last_is_lead=float(end.argmax() == 0))


for it in range(args.samples + 10):
    lib.th_memcpy_h2d(ctx.h, int(tick), tick0.ctypes.data, tick0.nbytes)
    for _ in range(args.steps):
        step()
    if lib.th_debug_tail_prof_all(ctx.h, buf.ctypes.data) != 0:
        sys.exit("th_debug_tail_prof_all failed")
    if SPLIT and lib.th_debug_tail_prof_op(ctx.h, buf_op.ctypes.data) != 0:
        sys.exit("th_debug_tail_prof_op failed")
    if it < 10:
        continue
    if SPLIT:
        rows.append(split_row(buf[:N_BLOCKS].astype(np.float64) * 0.01, buf_op[:N_BLOCKS].astype(np.float64) * 0.01))
        continue
    s = buf[:N_BLOCKS].astype(np.float64) * 0.01          # us
    start = s[:, 0].min()
    body, end, stepsz = s[:, 7] - s[:, 0], s[:, 7] - start, s[:, 2] - s[:, 1]
    dw = slice(N_HEAD, N_BLOCKS)
    row = {}
    for name, hi, lo in (("issue", 1, 0), ("wait", 3, 2), ("math", 5, 3), ("sync", 6, 5)):
        d = s[:, hi] - s[:, lo]
        row.update({f"lead_{name}": d[0], f"head_{name}": np.median(d[1:N_HEAD]), f"dw_{name}": np.median(d[dw])})
    rows.append(dict(row, lead_body=body[0], lead_end=end[0], lead_step=stepsz[0], lead_behind_barrier=s[0, 7] - s[0, 6],
                     head_body=np.median(body[1:N_HEAD]), head_end=np.median(end[1:N_HEAD]), head_behind_barrier=np.median(s[1:N_HEAD, 7] - s[1:N_HEAD, 6]),
                     dw_body=np.median(body[dw]), dw_end=np.median(end[dw]), dw_end_max=end[dw].max(), dw_step=np.median(stepsz[dw]),
                     launch=end.max(), last_is_lead=float(end.argmax() == 0)))
out = {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0] if k not in ("last_is_lead", "last_block")}
if SPLIT:
    out["last_is_head_frac"] = round(float(np.mean([0 < r["last_block"] < N_HEAD for r in rows])), 3)
out["last_is_lead_frac"] = round(float(np.mean([r["last_is_lead"] for r in rows])), 3)
out["lead_end_minus_dw_end_median"] = round(float(np.median([r["lead_end"] - r["dw_end"] for r in rows])), 3)
out["lead_end_minus_dw_end_max"] = round(float(np.median([r["lead_end"] - r["dw_end_max"] for r in rows])), 3)
# run-to-run spread of the figure the decision rests on: the medians of five equal parts of the samples
parts = np.array_split(np.array([r["lead_end"] - r["dw_end"] for r in rows]), 5)
out["lead_minus_dw_spread_of_5"] = round(float(max(np.median(p) for p in parts) - min(np.median(p) for p in parts)), 3)
out["samples"], out["t0"], out["split"] = len(rows), args.t0, int(SPLIT)
for k, v in out.items():
    print(f"{k:32s} {v}")
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(json.dumps(out, indent=1) + "\n")
