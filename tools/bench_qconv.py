"""Calibrated int8 convolution (th_quantize_act_nhwc_int8 + th_conv2d_q8q8_fwd) beside the weight-only int8 convolution (th_dequantize_multi +
th_conv3x3_fwd) and the f32 convolution (th_conv3x3_fwd), MI355X, timed in one process.

"int8 static per-channel" / "... chain per-channel" are the static rows with one weight pair per output channel (th_conv2d_q8q8_fwd_pc,
th_conv2d_q8q8_fwd_codes_pc, Module.quantize_static_per_channel: DESIGN 6m).

Layer rows: every Conv2dReLU(3x3, pad 1) of the reference CNN and of the simple CNN at B = 256, on its own, through the C ABI: us per forward in
two states -- cold (a 512 MiB buffer written elsewhere before every timed call) and graph-replayed (the forward captured once, the graph
launched back to back) -- and, for the static rows, the share of the two bounds of DESIGN 6k: integer operations against the i8 MFMA rate and
algorithmic bytes against 8 TB/s.

Pair rows: two consecutive static convs of the reference CNN at B = 256 (with the MaxPool2d(2) between them where the model has one), from
the first conv's codes to the second conv's f32 output, graph-replayed and cold as the layer rows: unchained = product, [f32 pool,] codec,
product; chained = product that writes codes (th_conv2d_q8q8_fwd_codes), [pool on codes (th_maxpool2d_nhwc_int8),] product.

Model rows: the whole forward of both models at B = 1, 64 and 256 for the float model, quantize("int8"), quantize_static,
quantize_static_conv and quantize_static_chain (checked bit-identical to quantize_static_conv's output on the timed input), through the
host library as a user calls it: cold as above, and "back to back" = the mean of eager calls issued without
a wait between them.  These rows are NOT graph replays: they time what a caller of the host library gets, tensor allocation and launch
work included, for all five models alike, so at B = 1 and 64 they say more about launches than about kernels; the layer and pair rows are
the kernel comparison.

    python tools/bench_qconv.py [--reps 30] [--out profiles/quant_static_conv.json]
    python tools/bench_qconv.py --kinds "int8 static,int8 static per-channel" --models cnn_reference      # a part of the rows
    python tools/bench_qconv.py --trace-only [--trace-kind "int8 static chain"]      # a few B = 256 forwards of the reference CNN's static-conv
                                                  # (or another) twin, for rocprofv3 --kernel-trace --stats

writes the rows as JSON to --out and the table beside it (same name, .md).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bench  # noqa: E402
import taper_amd as T  # noqa: E402
from oracle import train_extra as OX  # noqa: E402
from taper_amd import hip as H  # noqa: E402
from taper_amd._lib import hip as LIB  # noqa: E402

HBM = 8e12
I8_OPS = 2 * 2.5e15      # MI355X_MICROARCH: the i8 MFMA forms run at twice the bf16 rate per clock; bf16 dense peak ~2.5 PF
# (model, c_in, c_out, map side): the 3x3 / pad 1 layers of bench.build_model's two CNNs on 28 x 28 inputs
LAYERS = [("cnn_reference", 1, 32, 28), ("cnn_reference", 32, 32, 28), ("cnn_reference", 32, 64, 14), ("cnn_reference", 64, 64, 14),
          ("cnn_reference", 64, 128, 7), ("cnn_simple", 1, 32, 28), ("cnn_simple", 32, 64, 14)]
KINDS = ("f32", "int8 weight-only", "int8 static", "int8 static per-channel")
# (c_in, c_mid, c_out, map side of the first conv, a MaxPool2d(2) between the two): the reference CNN's consecutive static convs
PAIRS = [(1, 32, 32, 28, False), (32, 32, 64, 28, True), (32, 64, 64, 14, False), (64, 64, 128, 14, True)]
PAIR_KINDS = ("int8 static", "int8 static chain", "int8 static per-channel", "int8 static chain per-channel")


class Layer:
    """one 3x3 / pad 1 Conv2dReLU's operands on the device in the three forms"""

    def __init__(self, ctx, rng, c_in, c_out, side, B):
        s = np.sqrt(2.0 / (9 * c_in))
        w = rng.uniform(-s, s, (c_out, c_in, 3, 3)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, c_out).astype(np.float32)
        self.c_in, self.c_out, self.side, self.B = c_in, c_out, side, B
        self.w, self.b = ctx.upload(w), ctx.upload(b)
        q, sc, _, mn = OX.quantize_int8(w)
        qb, sb, _, mb = OX.quantize_int8(b)
        self.qw, self.qb = ctx.upload(q.view(np.uint8)), ctx.upload(qb.view(np.uint8))
        self.qwp, self.qbp = ctx.upload(np.array([mn, sc], np.float32)), ctx.upload(np.array([mb, sb], np.float32))
        self.cpitch = LIB.th_qconv_i8_cpitch(c_in)
        self.qw_nhwc = ctx.empty(c_out * 9 * self.cpitch, np.uint8)
        ctx.call("th_pack_conv_weight_taper_int8", self.qw, c_out, c_in, 3, 3, self.qw_nhwc, self.cpitch)
        self.sx = ctx.upload(np.array([4.0 / 127], np.float32))      # N(0, 1) inputs: a range of 4 sigma
        self.qx, self.ps = ctx.empty(B * side * side * self.cpitch, np.uint8), ctx.empty(B * side * side, np.int32)
        self.wf, self.bf = ctx.empty(w.size), ctx.empty(b.size)      # the weight-only twin's dequantize workspace
        self.items = (H.QTensor * 2)(H.QTensor(int(self.qw), int(self.qwp), int(self.wf), w.size, 0), H.QTensor(int(self.qb), int(self.qbp), int(self.bf), b.size, 0))
        self.x = ctx.upload(rng.standard_normal((B, c_in, side, side)).astype(np.float32))
        self.y = ctx.empty(B * c_out * side * side)
        self.qw_nhwc_pc = None

    def per_channel(self, ctx):
        """the weight packed again with a pair per effective output channel, on the device (once, when a per-channel row is first timed)"""
        if self.qw_nhwc_pc is None:
            qw = ctx.empty(self.c_out * self.c_in * 9, np.uint8)
            self.qwp_pc, self.qw_nhwc_pc = ctx.empty(2 * self.c_out), ctx.empty(self.c_out * 9 * self.cpitch, np.uint8)
            ctx.call("th_quantize_int8_channels", self.w, self.c_out, self.c_in * 9, 1, self.c_out, qw, self.qwp_pc)
            ctx.call("th_pack_conv_weight_taper_int8", qw, self.c_out, self.c_in, 3, 3, self.qw_nhwc_pc, self.cpitch)
            ctx.sync()

    def run(self, ctx, kind):
        B, s = self.B, self.side
        if kind == "f32":
            ctx.call("th_conv3x3_fwd", self.x, self.w, self.b, self.y, B, self.c_in, s, s, self.c_out, 1, 0, 1)
        elif kind == "int8 weight-only":
            ctx.call("th_dequantize_multi", C.addressof(self.items), 2)
            ctx.call("th_conv3x3_fwd", self.x, self.wf, self.bf, self.y, B, self.c_in, s, s, self.c_out, 1, 0, 1)
        elif kind == "int8 static per-channel":
            self.per_channel(ctx)
            ctx.call("th_quantize_act_nhwc_int8", self.x, B, self.c_in, s, s, self.sx, self.qx, self.cpitch, self.ps)
            ctx.call("th_conv2d_q8q8_fwd_pc", self.qx, self.cpitch, self.ps, self.sx, B, self.c_in, s, s, self.qw_nhwc_pc, self.c_out, 3, 3, 1, 1, 1, 1, self.qwp_pc,
                     self.qb, self.qbp, 1, self.y)
        else:
            ctx.call("th_quantize_act_nhwc_int8", self.x, B, self.c_in, s, s, self.sx, self.qx, self.cpitch, self.ps)
            ctx.call("th_conv2d_q8q8_fwd", self.qx, self.cpitch, self.ps, self.sx, B, self.c_in, s, s, self.qw_nhwc, self.c_out, 3, 3, 1, 1, 1, 1, self.qwp,
                     self.qb, self.qbp, 1, self.y)

    def static_bytes(self):
        """codec: x in, codes and pixel sums out; product: codes, pixel sums, channel-last weight codes in, y out"""
        px = self.B * self.side * self.side
        return 4 * px * self.c_in + 2 * px * self.cpitch + 8 * px + self.c_out * 9 * self.cpitch + 4 * px * self.c_out

    def ops(self):
        return 2 * self.B * self.side * self.side * 9 * self.c_in * self.c_out


class Pair:
    """conv A, [MaxPool2d(2),] conv B on the device: A's codes are made once, the timed part runs from them to B's f32 output"""

    def __init__(self, ctx, rng, c_in, c_mid, c_out, side, pool, B):
        self.a = Layer(ctx, rng, c_in, c_mid, side, B)
        self.b = Layer(ctx, rng, c_mid, c_out, side // 2 if pool else side, B)
        self.pool, self.B, self.side = pool, B, side
        self.b.sx = ctx.upload(np.array([2.0 / 127], np.float32))      # ReLU outputs of a He-initialised layer on N(0, 1) inputs: about 4 sigma
        ctx.call("th_quantize_act_nhwc_int8", self.a.x, B, c_in, side, side, self.a.sx, self.a.qx, self.a.cpitch, self.a.ps)
        if pool:
            self.mid_f32, self.argmax = ctx.empty(B * c_mid * (side // 2) ** 2), ctx.empty(B * c_mid * (side // 2) ** 2, np.int64)
            self.mid_q = ctx.empty(B * side * side * self.b.cpitch, np.uint8)

    def run(self, ctx, kind):
        a, b, B, s = self.a, self.b, self.B, self.side
        pc = "_pc" if kind.endswith("per-channel") else ""
        if pc:
            a.per_channel(ctx), b.per_channel(ctx)
        (qwa, qwpa), (qwb, qwpb) = ((l.qw_nhwc_pc, l.qwp_pc) if pc else (l.qw_nhwc, l.qwp) for l in (a, b))
        head = (a.qx, a.cpitch, a.ps, a.sx, B, a.c_in, s, s, qwa, a.c_out, 3, 3, 1, 1, 1, 1, qwpa, a.qb, a.qbp, 1)
        if "chain" not in kind:
            ctx.call("th_conv2d_q8q8_fwd" + pc, *head, a.y)
            if self.pool:
                ctx.call("th_maxpool2d_fwd", a.y, self.mid_f32, self.argmax, B, a.c_out, s, s, 2, 2, 2, 2, 0, 0)
            ctx.call("th_quantize_act_nhwc_int8", self.mid_f32 if self.pool else a.y, B, b.c_in, b.side, b.side, b.sx, b.qx, b.cpitch, b.ps)
        elif self.pool:
            ctx.call("th_conv2d_q8q8_fwd_codes" + pc, *head, b.sx, self.mid_q, b.cpitch, None)
            ctx.call("th_maxpool2d_nhwc_int8", self.mid_q, B, b.c_in, s, s, b.cpitch, 2, 2, 2, 2, 0, 0, b.qx, b.ps)
        else:
            ctx.call("th_conv2d_q8q8_fwd_codes" + pc, *head, b.sx, b.qx, b.cpitch, b.ps)
        ctx.call("th_conv2d_q8q8_fwd" + pc, b.qx, b.cpitch, b.ps, b.sx, B, b.c_in, b.side, b.side, qwb, b.c_out, 3, 3, 1, 1, 1, 1, qwpb, b.qb, b.qbp, 1, b.y)

    def output(self, ctx):
        return ctx.download(self.b.y, (self.B * self.b.c_out * self.b.side ** 2,)).view(np.uint32)


def timed(ctx, fn, reps, flush):
    """bench_qstatic.py's: (median cold us, us per graph replay)"""
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


def timed_eager(ctx, fn, reps, flush):
    """(median cold us, us per call of `reps` eager calls issued back to back)"""
    e0, e1 = H.Event(), H.Event()
    for _ in range(3):
        fn()
    ctx.sync()
    cold = []
    for _ in range(reps):
        ctx.call("th_fill_f32", flush, 1.0, 128 << 20)
        ctx.record(e0)
        fn()
        ctx.record(e1)
        cold.append(ctx.elapsed_ms(e0, e1) * 1e3)
    ctx.sync()
    ctx.record(e0)
    for _ in range(reps):
        fn()
    ctx.record(e1)
    warm = ctx.elapsed_ms(e0, e1) * 1e3 / reps
    ctx.sync()
    return statistics.median(cold), warm


def model_forwards(key, B, rng):
    """-> {kind: a call that runs one forward} for the five models of one network, calibrated on inputs like the timed ones"""
    model = bench.build_model(T, key)
    shape = (B, 1, 28, 28)
    calib = T.Tensor(rng.standard_normal((64, 1, 28, 28)).astype(np.float32), (64, 1, 28, 28))
    x = T.Tensor(rng.standard_normal(shape).astype(np.float32), shape)
    twins = {"int8 weight-only": model.quantize("int8"), "int8 static (Linear)": model.quantize_static(calib),
             "int8 static (conv + Linear)": model.quantize_static_conv(calib), "int8 static chain": model.quantize_static_chain(calib),
             "int8 static chain per-channel": model.quantize_static_per_channel(calib)}
    same = np.array_equal(twins["int8 static chain"](x).data().view(np.uint32), twins["int8 static (conv + Linear)"](x).data().view(np.uint32))
    assert same, f"{key} B={B}: the chained twin's output differs from quantize_static_conv's"
    same = np.array_equal(twins["int8 static chain per-channel"](x).data().view(np.uint32),
                          model.quantize_static_per_channel(calib, chain=False)(x).data().view(np.uint32))
    assert same, f"{key} B={B}: the chained per-channel twin's output differs from the unchained one's"

    def float_forward():
        model.forward(x)
        T.Tape.reset()

    calls = {"f32": float_forward}
    for kind, q in twins.items():
        calls[kind] = (lambda q: lambda: q(x))(q)
    return calls, (model, twins, x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="profiles/quant_static_conv.json")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--trace-kind", default="int8 static (conv + Linear)")
    ap.add_argument("--kinds", default="", help="comma-separated kinds to time (default: all)")
    ap.add_argument("--models", default="cnn_reference,cnn_simple", help="the models of the layer and model rows")
    ap.add_argument("--batches", default="1,64,256", help="the batch sizes of the model rows")
    a = ap.parse_args()

    def chosen(kind):
        return not a.kinds or kind in a.kinds.split(",")

    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    if a.trace_only:
        calls, keep = model_forwards("cnn_reference", 256, rng)
        for _ in range(5):
            calls[a.trace_kind]()
        ctx.sync()
        return
    flush = ctx.empty(128 << 20)
    rows = []

    def report(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    B = 256
    for key, c_in, c_out, side in (l for l in LAYERS if l[0] in a.models.split(",")):
        layer = Layer(ctx, rng, c_in, c_out, side, B)
        for kind in filter(chosen, KINDS):
            cold, warm = timed(ctx, lambda: layer.run(ctx, kind), a.reps, flush)
            r = dict(case=f"{key} conv {c_in}->{c_out} @ {side}x{side}", kind=kind, B=B, cold_us=round(cold, 2), replay_us=round(warm, 2))
            if kind.startswith("int8 static"):
                r.update(replay_share_of_i8_mfma=round(layer.ops() / (warm * 1e-6) / I8_OPS, 4),
                         replay_share_of_hbm=round(layer.static_bytes() / (warm * 1e-6) / HBM, 4))
            report(r)
        del layer
    for c_in, c_mid, c_out, side, pool in PAIRS:
        pair = Pair(ctx, rng, c_in, c_mid, c_out, side, pool, B)
        outs = {}
        for kind in filter(chosen, PAIR_KINDS):
            cold, warm = timed(ctx, lambda: pair.run(ctx, kind), a.reps, flush)
            outs[kind] = pair.output(ctx)
            report(dict(case=f"cnn_reference pair {c_in}->{c_mid} @ {side}x{side}{' -> pool' if pool else ''} -> {c_mid}->{c_out}", kind=kind, B=B,
                        cold_us=round(cold, 2), replay_us=round(warm, 2)))
        for pc in (False, True):      # per codec, a chained pair computes what its unchained pair computes
            same = [o for k, o in outs.items() if k.endswith("per-channel") == pc]
            assert all(np.array_equal(same[0], o) for o in same), "the chained pair's output differs from the unchained pair's"
        del pair
    for key in a.models.split(","):
        for B in map(int, a.batches.split(",")):
            calls, keep = model_forwards(key, B, rng)
            for kind, fn in ((k, f) for k, f in calls.items() if chosen(k)):
                cold, warm = timed_eager(ctx, fn, a.reps, flush)
                report(dict(case=f"{key} forward", kind=kind, B=B, cold_us=round(cold, 2), back_to_back_us=round(warm, 2)))
            del calls, keep

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))
    out.with_suffix(".md").write_text(table(rows, a.reps))


def table(rows, reps):
    lines = [f"# Calibrated int8 convolution on MI355X (`tools/bench_qconv.py`, {reps} reps; cold = median after writing 512 MiB elsewhere)", "",
             "Layer rows (C ABI, replay = the captured forward launched back to back): static = `th_quantize_act_nhwc_int8` + `th_conv2d_q8q8_fwd`; "
             "weight-only = `th_dequantize_multi` + `th_conv3x3_fwd`; f32 = `th_conv3x3_fwd`.",
             "Pair rows (C ABI, replay, from the first conv's codes to the second conv's f32 output): static = product, [f32 pool,] codec, product; "
             "static chain = `th_conv2d_q8q8_fwd_codes`, [`th_maxpool2d_nhwc_int8`,] product -- the same output bits, asserted.  per-channel: the "
             "same launches through the `_pc` entry points, one weight pair per output channel.",
             "Shares (static rows, replay): integer operations / time / 5 POPS (twice the bf16 matrix peak), algorithmic bytes / time / 8 TB/s.",
             "Model rows (host library, eager, not graph replays: tensor allocation and launch work included for all models alike): back to back = "
             "the mean of calls issued without a wait between them.",
             "", "| case | kind | B | cold µs | replay / back-to-back µs | share of i8 MFMA | share of HBM |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['kind']} | {r['B']} | {r['cold_us']} | {r.get('replay_us', r.get('back_to_back_us'))} | "
                     f"{r.get('replay_share_of_i8_mfma', '')} | {r.get('replay_share_of_hbm', '')} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
