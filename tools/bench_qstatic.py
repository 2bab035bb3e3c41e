"""Calibrated int8 Linear forward (th_quantize_act_int8 + th_linear_q8q8_fwd) beside the weight-only int8 forward (th_linear_q8_fwd) and the
f32 forward (th_linear_fwd), MI355X, timed in one process; "int8 static per-channel" is the same forward with one weight pair per output
row (th_linear_q8q8_fwd_pc), and the codec rows time th_quantize_int8_channels beside th_quantize_int8 on the same buffers.

Rows: a 4096 x 4096 layer at B = 1, 8, 64, 256, 257, 512, 4096, and the 4 x 4096^2 + classifier stack at B = 4096.  Each row: us per forward in two
states -- cold (a 512 MiB buffer written elsewhere before every timed call) and graph-replayed (the forward captured once, the graph
launched back to back) -- and, for the static rows, the share of the two bounds of DESIGN 6j: integer operations against the i8 MFMA rate
(2 x the 2.5 PF bf16 peak) and algorithmic bytes against 8 TB/s.

    python tools/bench_qstatic.py [--reps 30] [--out profiles/quant_static.json]
    python tools/bench_qstatic.py --kinds "int8 static,int8 static per-channel" --batches 1,64,4096 --skip-stack      # a part of the rows
    python tools/bench_qstatic.py --trace-only      # a few static B = 4096 forwards and nothing else, for rocprofv3 --kernel-trace --stats

writes the rows as JSON to --out and the table beside it (same name, .md).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import taper_amd as T  # noqa: E402
from oracle import train_extra as OX  # noqa: E402
from taper_amd import hip as H  # noqa: E402
from taper_amd._lib import hip as LIB  # noqa: E402

HBM = 8e12
I8_OPS = 2 * 2.5e15      # MI355X_MICROARCH: the i8 MFMA forms run at twice the bf16 rate per clock; bf16 dense peak ~2.5 PF


class Layer:
    """one Linear's operands on the device in the three forms"""

    def __init__(self, ctx, rng, K, N, max_b):
        s = np.sqrt(2.0 / K)
        w = rng.uniform(-s, s, (N, K)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, N).astype(np.float32)
        self.K, self.N = K, N
        self.w, self.b = ctx.upload(w), ctx.upload(b)
        q, sc, _, mn = OX.quantize_int8(w)
        qb, sb, _, mb = OX.quantize_int8(b)
        self.qw, self.qb = ctx.upload(q.view(np.uint8)), ctx.upload(qb.view(np.uint8))
        self.qwp, self.qbp = ctx.upload(np.array([mn, sc], np.float32)), ctx.upload(np.array([mb, sb], np.float32))
        step = LIB.th_qlinear_i8_kstep()
        self.pitch_w, self.pitch_x = -(-K // step) * step, -(-K // 16) * 16
        self.qw_pad = ctx.empty(N * self.pitch_w, np.uint8)
        ctx.call("th_pad_rows_int8", self.qw, N, K, self.qw_pad, self.pitch_w)
        self.sx = ctx.upload(np.array([4.0 / 127], np.float32))      # N(0, 1) inputs: a range of 4 sigma
        self.qx, self.rs = ctx.empty(max_b * self.pitch_x, np.uint8), ctx.empty(max_b, np.int32)
        self.qw_pad_pc = None

    def per_channel(self, ctx):
        """the weight packed again with a pair per row, on the device (once, when a per-channel row is first timed)"""
        if self.qw_pad_pc is None:
            qw = ctx.empty(self.N * self.K, np.uint8)
            self.qwp_pc, self.qw_pad_pc = ctx.empty(2 * self.N), ctx.empty(self.N * self.pitch_w, np.uint8)
            ctx.call("th_quantize_int8_channels", self.w, self.N, self.K, self.K, 1, qw, self.qwp_pc)
            ctx.call("th_pad_rows_int8", qw, self.N, self.K, self.qw_pad_pc, self.pitch_w)
            ctx.sync()

    def run(self, ctx, kind, x, y, B, relu=0):
        if kind == "f32":
            ctx.call("th_linear_fwd", x, self.w, self.b, y, B, self.K, self.N, relu)
        elif kind == "int8 weight-only":
            ctx.call("th_linear_q8_fwd", x, B, self.K, self.qw, self.N, self.qwp, self.qb, self.qbp, relu, y)
        elif kind == "int8 static per-channel":
            self.per_channel(ctx)
            ctx.call("th_quantize_act_int8", x, B, self.K, self.sx, self.qx, self.pitch_x, self.rs)
            ctx.call("th_linear_q8q8_fwd_pc", self.qx, self.pitch_x, self.rs, self.sx, B, self.K, self.qw_pad_pc, self.pitch_w, self.N, self.qwp_pc, self.qb,
                     self.qbp, relu, y)
        else:
            ctx.call("th_quantize_act_int8", x, B, self.K, self.sx, self.qx, self.pitch_x, self.rs)
            ctx.call("th_linear_q8q8_fwd", self.qx, self.pitch_x, self.rs, self.sx, B, self.K, self.qw_pad, self.pitch_w, self.N, self.qwp, self.qb,
                     self.qbp, relu, y)

    def static_bytes(self, B):
        """quantize: x in, codes and row sums out; product: codes, row sums, padded weight codes, bias in, y out"""
        return 4 * B * self.K + 2 * B * self.pitch_x + 8 * B + self.N * self.pitch_w + self.N + 4 * B * self.N

    def ops(self, B):
        return 2 * B * self.K * self.N


KINDS = ("f32", "int8 weight-only", "int8 static", "int8 static per-channel")


def timed(ctx, fn, reps, flush):
    e0, e1 = H.Event(), H.Event()
    fn()
    ctx.sync()
    cold = []
    for _ in range(reps):
        ctx.call("th_fill_f32", flush, 1.0, 128 << 20)   # 512 MiB written elsewhere: the layer's bytes leave L2 and the Infinity Cache
        ctx.record(e0)
        fn()
        ctx.record(e1)
        cold.append(ctx.elapsed_ms(e0, e1) * 1e3)
    ctx.graph_begin()
    fn()
    g = ctx.graph_end()
    ctx.graph_launch(g)
    ctx.sync()
    ctx.record(e0)
    for _ in range(reps):
        ctx.graph_launch(g)
    ctx.record(e1)
    replay = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    ctx.sync()
    ctx.graph_destroy(g)
    return statistics.median(cold), replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="profiles/quant_static.json")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kinds", default=",".join(KINDS), help="comma-separated kinds to time")
    ap.add_argument("--batches", default="1,8,64,256,257,512,4096")
    ap.add_argument("--skip-stack", action="store_true")
    a = ap.parse_args()
    kinds = [k for k in KINDS if k in a.kinds.split(",")]
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    BIG = 4096
    layer = Layer(ctx, rng, 4096, 4096, BIG)
    xbig = ctx.upload(rng.standard_normal((BIG, 4096)).astype(np.float32))
    ybig = ctx.empty(BIG * 4096)
    if a.trace_only:
        for _ in range(5):
            layer.run(ctx, "int8 static", xbig, ybig, BIG)
        ctx.sync()
        return
    flush = ctx.empty(128 << 20)
    rows = []

    def report(name, kind, B, cold, warm, ops, nbytes):
        r = dict(case=name, kind=kind, B=B, cold_us=round(cold, 2), replay_us=round(warm, 2))
        if kind.startswith("int8 static"):
            r.update(replay_share_of_i8_mfma=round(ops / (warm * 1e-6) / I8_OPS, 4), replay_share_of_hbm=round(nbytes / (warm * 1e-6) / HBM, 4))
        rows.append(r)
        print(json.dumps(r), flush=True)

    for B in map(int, a.batches.split(",")):      # 256 / 257: both sides of the switch between the product's two forms
        for kind in kinds:
            cold, warm = timed(ctx, lambda: layer.run(ctx, kind, xbig, ybig, B), a.reps, flush)
            report("linear 4096x4096", kind, B, cold, warm, layer.ops(B), layer.static_bytes(B))

    if "int8 static per-channel" in kinds:
        codec_rows(ctx, rng, a.reps, flush, report)
    stack = [] if a.skip_stack else [layer] + [Layer(ctx, rng, 4096, 4096, BIG) for _ in range(3)] + [Layer(ctx, rng, 4096, 10, BIG)]
    xs = [xbig, ybig] + [ctx.empty(BIG * 4096) for _ in range(3)] + [ctx.empty(BIG * 10)]
    for kind in kinds if stack else ():
        def fwd():
            for i, l in enumerate(stack):
                l.run(ctx, kind, xs[i], xs[i + 1], BIG, relu=1 if i < 4 else 0)
        cold, warm = timed(ctx, fwd, max(5, a.reps // 3), flush)
        report("stack 4x4096^2 + 4096x10", kind, BIG, cold, warm, sum(l.ops(BIG) for l in stack), sum(l.static_bytes(BIG) for l in stack))

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))
    out.with_suffix(".md").write_text(table(rows, a.reps))


def codec_rows(ctx, rng, reps, flush, report):
    """th_quantize_int8_channels on a 4096^2 weight by rows and on a 128-channel 3x3 conv buffer ([1152][128]) by columns, each beside
    th_quantize_int8 on the same buffers"""
    for name, channels, ln, rows in (("4096x4096 rows", 4096, 4096, True), ("1152x128 columns", 128, 1152, False)):
        n = channels * ln
        x, q, p = ctx.upload(rng.standard_normal(n).astype(np.float32)), ctx.empty(n, np.uint8), ctx.empty(2 * channels)
        strides = (ln, 1) if rows else (1, channels)
        for kind, fn in (("th_quantize_int8", lambda: ctx.call("th_quantize_int8", x, q, n, p)),
                         ("th_quantize_int8_channels", lambda: ctx.call("th_quantize_int8_channels", x, channels, ln, *strides, q, p))):
            cold, warm = timed(ctx, fn, reps, flush)
            report("codec " + name, kind, channels, cold, warm, 0, 0)


def table(rows, reps):
    lines = [f"# Calibrated int8 Linear forward on MI355X (`tools/bench_qstatic.py`, {reps} reps; cold = median after writing 512 MiB elsewhere, "
             "replay = the captured forward launched back to back)", "",
             "static = `th_quantize_act_int8` + `th_linear_q8q8_fwd` (two launches); static per-channel = the same with `th_linear_q8q8_fwd_pc`; "
             "weight-only = `th_linear_q8_fwd`; f32 = `th_linear_fwd`.  Codec rows: one call on the buffer, B = its channels.",
             "Shares (static rows, replay): integer operations / time / 5 POPS (twice the bf16 matrix peak), algorithmic bytes / time / 8 TB/s.",
             "", "| case | kind | B | cold µs | replay µs | share of i8 MFMA | share of HBM |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['kind']} | {r['B']} | {r['cold_us']} | {r['replay_us']} | {r.get('replay_share_of_i8_mfma', '')} | "
                     f"{r.get('replay_share_of_hbm', '')} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
