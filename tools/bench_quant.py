"""Quantized Linear forward (th_linear_q8_fwd / th_linear_h16_fwd) beside the f32 forward (th_linear_fwd), MI355X.

Rows: (K, N) = (4096, 4096) and (784, 128) at B = 1, 4, 8, 16, 64; the 4 x 4096^2 + classifier stack at B = 1 and 8; the quantized reference
CNN at B = 64 (through the Python face).  Each row: us per forward, algorithmic bytes (weights + bias + x + y) and their share of the
8 TB/s HBM bound, in two cache states -- cold (a 512 MiB buffer written elsewhere before every timed call) and replayed (back to back).

    python tools/bench_quant.py [--reps 50] [--out profiles/quant_linear.json]

writes the rows as JSON to --out and the table beside it (same name, .md): the committed summary is profiles/quant_linear.{json,md}.
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

HBM = 8e12


class Layer:
    def __init__(self, ctx, rng, K, N):
        s = np.sqrt(2.0 / K)
        w = rng.uniform(-s, s, (N, K)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, N).astype(np.float32)
        self.K, self.N = K, N
        self.w, self.b = ctx.upload(w), ctx.upload(b)
        q, sc, _, mn = OX.quantize_int8(w)
        qb, sb, _, mb = OX.quantize_int8(b)
        self.qw, self.qb = ctx.upload(q.view(np.uint8)), ctx.upload(qb.view(np.uint8))
        self.qwp, self.qbp = ctx.upload(np.array([mn, sc], np.float32)), ctx.upload(np.array([mb, sb], np.float32))
        self.hw, self.hb = ctx.upload(OX.f32_to_f16_bits(w)), ctx.upload(OX.f32_to_f16_bits(b))

    def wbytes(self, kind):
        return {"f32": 4, "int8": 1, "f16": 2}[kind] * (self.K * self.N + self.N) + (16 if kind == "int8" else 0)

    def run(self, ctx, kind, x, y, B, relu=0):
        if kind == "f32":
            ctx.call("th_linear_fwd", x, self.w, self.b, y, B, self.K, self.N, relu)
        elif kind == "int8":
            ctx.call("th_linear_q8_fwd", x, B, self.K, self.qw, self.N, self.qwp, self.qb, self.qbp, relu, y)
        else:
            ctx.call("th_linear_h16_fwd", x, B, self.K, self.hw, self.N, self.hb, relu, y)


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
    ctx.record(e0)
    for _ in range(reps):
        fn()
    ctx.record(e1)
    return statistics.median(cold), ctx.elapsed_ms(e0, e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="profiles/quant_linear.json")
    a = ap.parse_args()
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(name, kind, B, nbytes, cold, warm):
        r = dict(case=name, kind=kind, B=B, bytes=nbytes, cold_us=round(cold, 2), replay_us=round(warm, 2),
                 cold_bw_share=round(nbytes / (cold * 1e-6) / HBM, 3), replay_bw_share=round(nbytes / (warm * 1e-6) / HBM, 3))
        rows.append(r)
        print(json.dumps(r), flush=True)

    for K, N in ((4096, 4096), (784, 128)):
        layer = Layer(ctx, rng, K, N)
        for B in (1, 4, 8, 16, 64):
            x, y = ctx.upload(rng.standard_normal((B, K)).astype(np.float32)), ctx.empty(B * N)
            for kind in ("f32", "int8", "f16"):
                cold, warm = timed(ctx, lambda: layer.run(ctx, kind, x, y, B), a.reps, flush)
                report(f"linear {K}x{N}", kind, B, layer.wbytes(kind) + 4 * B * (K + N), cold, warm)

    stack = [Layer(ctx, rng, 4096, 4096) for _ in range(4)] + [Layer(ctx, rng, 4096, 10)]
    for B in (1, 8):
        xs = [ctx.upload(rng.standard_normal((B, 4096)).astype(np.float32))] + [ctx.empty(B * 4096) for _ in range(4)] + [ctx.empty(B * 10)]
        for kind in ("f32", "int8", "f16"):
            def fwd():
                for i, l in enumerate(stack):
                    l.run(ctx, kind, xs[i], xs[i + 1], B, relu=1 if i < 4 else 0)
            nbytes = sum(l.wbytes(kind) + 4 * B * (l.K + l.N) for l in stack)
            cold, warm = timed(ctx, fwd, a.reps, flush)
            report("stack 4x4096^2 + 4096x10", kind, B, nbytes, cold, warm)

    from tests import backends
    spec = backends.cnn_reference(np.random.default_rng(1))
    model = backends.HipBackend().sequential(spec)
    n_params = sum(p.numel() for p in model.parameters())
    B = 64
    x = T.Tensor(rng.uniform(0, 1, (B, 784)).astype(np.float32), (B, 1, 28, 28))
    for kind in ("f32", "int8", "float16"):
        q = model.quantize(kind) if kind != "f32" else None

        def fwd():
            T.Tape.reset()
            return (q(x) if q else model.forward(x))
        nbytes = q.storage_bytes() if q else 4 * n_params
        cold, warm = timed(ctx, fwd, max(5, a.reps // 5), flush)
        report("reference CNN (Python face)", kind, B, nbytes, cold, warm)
    T.Tape.reset()

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))
    out.with_suffix(".md").write_text(table(rows, a.reps))


def table(rows, reps):
    lines = [f"# Quantized Linear forward on MI355X (`tools/bench_quant.py`, {reps} reps; cold = median after writing 512 MiB elsewhere, "
             "replay = back to back)", "",
             "Bytes are algorithmic (codes + {min, scale} + x + y); share = bytes / time / 8 TB/s.  B <= 8 takes the weight-streaming kernel,",
             "B > 8 dequantizes into a pooled workspace and runs `th_linear_fwd`.  The CNN row is the whole quantized forward through the Python face.",
             "", "| case | kind | B | bytes | cold µs | replay µs | cold share | replay share |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['kind']} | {r['B']} | {r['bytes']} | {r['cold_us']} | {r['replay_us']} | {r['cold_bw_share']} | "
                     f"{r['replay_bw_share']} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
