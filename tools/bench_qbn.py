"""A frozen BatchNorm2d in the int8 twins on MI355X, timed in one process.

Product rows (C ABI): one static conv's product from its codes, 3x3 / pad 1 at B = 256, per-channel weight pairs, in the f32 form and the
codes form: `_pc` (th_conv2d_q8q8_fwd_pc / _codes_pc) beside `_affine` (th_conv2d_q8q8_fwd_affine / _codes_affine with per_channel = 1), and
the unfused alternative `_pc + th_channel_affine_fwd` for the f32 form.  us per call in two states, as tools/bench_qconv.py measures them:
cold (a 512 MiB buffer written elsewhere before every timed call, median) and graph-replayed.  A library without the `_affine` entry points
(an older build of this project) gets the `_pc` rows alone: run the tool in both trees to compare builds.

Model rows (host library, eager: tensor allocation and launch work included): Sequential{BasicBlock(1, 32), BasicBlock(32, 32), MaxPool2d(2),
BasicBlock(32, 64), Flatten, Linear(64 * 14 * 14, 10)} on 28 x 28 inputs at B = 256 and B = 1 -- the float model in eval mode, quantize_static
(weight-only convs, standalone BatchNorm layers, a static Linear) and the chained per-channel twin; cold as above and back to back = the mean of calls issued without a wait between them.

    python tools/bench_qbn.py [--reps 30] [--tag NAME] [--out profiles/quant_batchnorm.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import taper_amd as T  # noqa: E402
from taper_amd import hip as H  # noqa: E402
from taper_amd._lib import hip as LIB  # noqa: E402
from tools.bench_qconv import timed, timed_eager  # noqa: E402

SHAPES = [(64, 64, 14), (32, 32, 28)]      # c_in, c_out, map side
HAS_AFFINE = hasattr(LIB, "th_conv2d_q8q8_fwd_affine")


class Product:
    """the operands of one static conv on the device: random codes (the time does not depend on their values), a pair per channel"""

    def __init__(self, ctx, rng, c_in, c_out, side, B):
        self.c_in, self.c_out, self.side, self.B = c_in, c_out, side, B
        px = B * side * side
        self.cpitch, self.cpitch_y = LIB.th_qconv_i8_cpitch(c_in), LIB.th_qconv_i8_cpitch(c_out)
        qx = rng.integers(-128, 128, (px, self.cpitch)).astype(np.int8)
        self.qx, self.ps = ctx.upload(qx.view(np.uint8)), ctx.upload(qx.astype(np.int32).sum(axis=1).astype(np.int32))
        self.qw = ctx.upload(rng.integers(-128, 128, (c_out, 9, self.cpitch)).astype(np.int8).view(np.uint8))
        self.qb, self.bp = ctx.upload(rng.integers(-128, 128, c_out).astype(np.int8).view(np.uint8)), ctx.upload(np.array([-0.1, 0.001], np.float32))
        self.sx, self.sy = ctx.upload(np.array([4.0 / 127], np.float32)), ctx.upload(np.array([2.0 / 127], np.float32))
        self.wp = ctx.upload(np.stack([np.full(c_out, -0.2, np.float32), np.linspace(1e-3, 2e-3, c_out).astype(np.float32)], axis=1))
        self.ab = ctx.upload(np.stack([np.linspace(0.5, 1.5, c_out).astype(np.float32), np.linspace(-0.1, 0.1, c_out).astype(np.float32)], axis=1))
        self.y, self.qy, self.yps = ctx.empty(px * c_out), ctx.empty(px * self.cpitch_y, np.uint8), ctx.empty(px, np.int32)

    def run(self, ctx, kind):
        s = self.side
        head = (self.qx, self.cpitch, self.ps, self.sx, self.B, self.c_in, s, s, self.qw, self.c_out, 3, 3, 1, 1, 1, 1, self.wp, self.qb, self.bp, 1)
        if kind == "_pc f32":
            ctx.call("th_conv2d_q8q8_fwd_pc", *head, self.y)
        elif kind == "_affine f32":
            ctx.call("th_conv2d_q8q8_fwd_affine", *head, self.y, 1, self.ab)
        elif kind == "_pc f32 + th_channel_affine_fwd":
            ctx.call("th_conv2d_q8q8_fwd_pc", *head[:-1], 0, self.y)
            ctx.call("th_channel_affine_fwd", self.y, self.ab, self.B, self.c_out, s * s, 1, self.y)
        elif kind == "_pc codes":
            ctx.call("th_conv2d_q8q8_fwd_codes_pc", *head, self.sy, self.qy, self.cpitch_y, self.yps)
        else:
            ctx.call("th_conv2d_q8q8_fwd_codes_affine", *head, self.sy, self.qy, self.cpitch_y, self.yps, 1, self.ab)


def block_model(rng):
    model = T.Sequential([T.BasicBlock(1, 32, seed=1), T.BasicBlock(32, 32, seed=2), T.MaxPool2d((2, 2), (2, 2)), T.BasicBlock(32, 64, seed=3), T.Flatten(1),
                          T.Linear(64 * 14 * 14, 10, True, seed=4)])
    model.train()
    for _ in range(3):      # running statistics of the model's own activations
        model.forward(T.Tensor(rng.standard_normal((64, 1, 28, 28)).astype(np.float32), (64, 1, 28, 28)))
    T.Tape.reset()
    model.eval()
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tag", default="this build")
    ap.add_argument("--out", default="profiles/quant_batchnorm.json")
    a = ap.parse_args()
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(r):
        r["build"] = a.tag
        rows.append(r)
        print(json.dumps(r), flush=True)

    kinds = ("_pc f32", "_affine f32", "_pc f32 + th_channel_affine_fwd", "_pc codes", "_affine codes") if HAS_AFFINE else ("_pc f32", "_pc codes")
    for c_in, c_out, side in SHAPES:
        p = Product(ctx, rng, c_in, c_out, side, 256)
        for kind in kinds:
            cold, warm = timed(ctx, lambda: p.run(ctx, kind), a.reps, flush)
            report(dict(case=f"product {c_in}->{c_out} @ {side}x{side}", kind=kind, B=256, cold_us=round(cold, 2), replay_us=round(warm, 2)))
        del p
    if HAS_AFFINE:
        model = block_model(rng)
        calib = T.Tensor(rng.standard_normal((64, 1, 28, 28)).astype(np.float32), (64, 1, 28, 28))
        twins = {"int8 static (Linear), convs weight-only": model.quantize_static(calib), "int8 static chain per-channel": model.quantize_static_per_channel(calib)}
        assert twins["int8 static chain per-channel"].chain_links() == 2
        for B in (256, 1):
            x = T.Tensor(rng.standard_normal((B, 1, 28, 28)).astype(np.float32), (B, 1, 28, 28))

            def float_forward():
                model.forward(x)
                T.Tape.reset()

            calls = {"f32 eval": float_forward}
            for kind, q in twins.items():
                calls[kind] = (lambda q: lambda: q(x))(q)
            fl = model.forward(x).data()
            T.Tape.reset()
            for kind, fn in calls.items():
                cold, warm = timed_eager(ctx, fn, a.reps, flush)
                r = dict(case="BasicBlock model forward", kind=kind, B=B, cold_us=round(cold, 2), back_to_back_us=round(warm, 2))
                if kind != "f32 eval":
                    r["err_over_max_abs_float"] = round(float(np.abs(twins[kind](x).data() - fl).max() / np.abs(fl).max()), 5)
                report(r)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
