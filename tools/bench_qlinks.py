"""Int8 links through the classifier (th_linear_q8q8_fwd_link, Module.quantize_static_linked: DESIGN 6o) on MI355X, timed in one process.

Parts (--parts, comma-separated):
    product  th_linear_q8q8_fwd alone on a 4096 x 4096 layer at B = 1, 64, 4096: the existing f32 product, to be set beside the same rows
             of another build of the library (the part needs nothing of the link, so it runs on a tree without it)
    rowsum   th_linear_q8q8_fwd_link with d_rowsum = NULL beside the same call with the sums given, on the same codes, f32 destination;
             and the codes destination beside the f32 one (sums given)
    twins    the linked twin beside the unlinked twin of the same build (same flags without the links; checked bit-identical on the timed
             input): a pair Linear(4096, 4096), ReLU, Linear(4096, 4096) at B = 1, 64, 4096, the 4 x 4096^2 + classifier stack at
             B = 4096, and the reference CNN (two Linear links; an average pool stands in front of its Flatten) and the simple CNN (the
             Flatten link) at B = 1, 256

Each row: us per call, cold (a 512 MiB buffer written elsewhere before every timed call, median), graph-replayed (captured once, launched
back to back) and, for the twins, eager calls issued back to back through the host library.

    python tools/bench_qlinks.py [--reps 30] [--parts product,rowsum,twins] [--out profiles/quant_links.json]

writes the rows as JSON to --out and prints each as it is measured.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bench  # noqa: E402
import taper_amd as T  # noqa: E402
from taper_amd import hip as H  # noqa: E402
from taper_amd._lib import host as HOST  # noqa: E402

CONVS, CHAIN, LINKS = 1, 2, 16


def timed(ctx, fn, reps, flush, replay=True):
    """bench_qstatic.py's, with the eager back-to-back figure beside it: (median cold us, us per eager call, us per graph replay or None)"""
    e0, e1 = H.Event(), H.Event()
    for _ in range(3):
        fn()
    ctx.sync()
    cold = []
    for _ in range(reps):
        ctx.call("th_fill_f32", flush, 1.0, 128 << 20)   # 512 MiB written elsewhere: the operands leave L2 and the Infinity Cache
        ctx.record(e0)
        fn()
        ctx.record(e1)
        cold.append(ctx.elapsed_ms(e0, e1) * 1e3)
    ctx.sync()
    ctx.record(e0)
    for _ in range(reps):
        fn()
    ctx.record(e1)
    eager = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    ctx.sync()
    if not replay:
        return statistics.median(cold), eager, None
    ctx.graph_begin()
    keep = fn()
    g = ctx.graph_end()
    ctx.graph_launch(g)
    ctx.sync()
    ctx.record(e0)
    for _ in range(reps):
        ctx.graph_launch(g)
    ctx.record(e1)
    warm = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    ctx.sync()
    del keep
    ctx.graph_destroy(g)
    return statistics.median(cold), eager, warm


class Codes:
    """a 4096 x 4096 layer's operands as codes on the device, the activation codes made by the library's own codec"""

    def __init__(self, ctx, rng, K, N, B):
        self.K, self.N, self.B = K, N, B
        s = np.sqrt(2.0 / K)
        qw = ctx.upload(rng.integers(-128, 128, (N, K)).astype(np.int8).view(np.uint8))      # K is a multiple of the K step: no padding
        self.qw, self.wp = qw, ctx.upload(np.array([-s, 2 * s / 255], np.float32))
        self.qb, self.bp = ctx.upload(rng.integers(-128, 128, N).astype(np.int8).view(np.uint8)), ctx.upload(np.array([-0.1, 0.2 / 255], np.float32))
        self.sx, self.sy = ctx.upload(np.array([4.0 / 127], np.float32)), ctx.upload(np.array([4.0 / 127], np.float32))
        x = ctx.upload(rng.standard_normal((B, K)).astype(np.float32))
        self.qx, self.rs = ctx.empty(B * K, np.uint8), ctx.empty(B, np.int32)
        ctx.call("th_quantize_act_int8", x, B, K, self.sx, self.qx, K, self.rs)
        self.y, self.qy = ctx.empty(B * N), ctx.empty(B * N, np.uint8)
        ctx.sync()

    def old(self, ctx, B):
        ctx.call("th_linear_q8q8_fwd", self.qx, self.K, self.rs, self.sx, B, self.K, self.qw, self.K, self.N, self.wp, self.qb, self.bp, 1, self.y)

    def link(self, ctx, B, own, codes):
        ctx.call("th_linear_q8q8_fwd_link", self.qx, self.K, None if own else self.rs, self.sx, B, self.K, self.qw, self.K, self.N, self.wp, 0, self.qb, self.bp, 1,
                 None if codes else self.y, self.sy, self.qy if codes else None, self.N if codes else 0)


def twin(model, calib, flags):
    return model._quantize_static(HOST.tp_module_quantize_static_ex, "quantize_static_ex", calib, flags)


def twin_rows(ctx, rng, reps, flush, report):
    def mlp(widths):
        layers = []
        for i, (k, n) in enumerate(zip(widths, widths[1:])):
            layers += [T.Linear(k, n, True, seed=i + 1)] + ([T.ReLU()] if i + 2 < len(widths) else [])
        return T.Sequential(layers)

    cases = [("pair 4096 -> 4096 -> 4096", mlp([4096] * 3), (4096,), (1, 64, 4096), 0),
             ("stack 4x4096^2 + 4096x10", mlp([4096] * 5 + [10]), (4096,), (4096,), 0),
             ("cnn_reference", bench.build_model(T, "cnn_reference"), (1, 28, 28), (1, 256), CONVS | CHAIN),      # (an average pool: no Flatten link)
             ("cnn_simple", bench.build_model(T, "cnn_simple"), (1, 28, 28), (1, 256), CONVS | CHAIN)]            # the Flatten link: 49 pixels x 64 channels
    for name, model, sample, batches, flags in cases:
        cshape = (64,) + sample
        calib = T.Tensor(rng.standard_normal(cshape).astype(np.float32), cshape)
        twins = {"unlinked": twin(model, calib, flags), "linked": twin(model, calib, flags | LINKS)}
        for B in batches:
            shape = (B,) + sample
            x = T.Tensor(rng.standard_normal(shape).astype(np.float32), shape)
            same = np.array_equal(twins["linked"](x).data().view(np.uint32), twins["unlinked"](x).data().view(np.uint32))
            assert same, f"{name} B={B}: the linked twin's output differs from the unlinked twin's"
            for kind, q in twins.items():
                cold, eager, warm = timed(ctx, lambda: q(x), reps, flush)
                report(dict(case=name, kind=kind, links=q.chain_links(), B=B, cold_us=round(cold, 2), eager_us=round(eager, 2), replay_us=round(warm, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parts", default="product,rowsum,twins")
    ap.add_argument("--out", default="profiles/quant_links.json")
    ap.add_argument("--tag", default="", help="a label for every row (the build, the round)")
    a = ap.parse_args()
    parts = a.parts.split(",")
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(r):
        if a.tag:
            r["tag"] = a.tag
        rows.append(r)
        print(json.dumps(r), flush=True)

    if "product" in parts or "rowsum" in parts:
        layer = Codes(ctx, rng, 4096, 4096, 4096)
        for B in (1, 64, 4096):
            calls = []
            if "product" in parts:
                calls.append(("th_linear_q8q8_fwd", lambda: layer.old(ctx, B)))
            if "rowsum" in parts:
                calls += [("link, sums given, f32", lambda: layer.link(ctx, B, False, False)), ("link, own sums, f32", lambda: layer.link(ctx, B, True, False)),
                          ("link, sums given, codes", lambda: layer.link(ctx, B, False, True)), ("link, own sums, codes", lambda: layer.link(ctx, B, True, True))]
            for kind, fn in calls:
                cold, eager, warm = timed(ctx, fn, a.reps, flush)
                report(dict(case="product 4096x4096", kind=kind, B=B, cold_us=round(cold, 2), eager_us=round(eager, 2), replay_us=round(warm, 2)))
    if "twins" in parts:
        twin_rows(ctx, rng, max(5, a.reps // 2), flush, report)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
