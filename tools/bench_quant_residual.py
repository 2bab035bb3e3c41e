"""Quantized residual models on MI355X, timed in one process.

Product rows (C ABI, graph-replayed and cold as tools/bench_qconv.py measures them): the residual product beside the composition it
replaces, per-channel weight pairs, B = 256:

    f32 form    th_conv2d_q8q8_fwd_residual                      vs   th_conv2d_q8q8_fwd_affine (no ReLU) + th_add + th_relu_fwd
    codes form  th_conv2d_q8q8_fwd_codes_residual                vs   the same three + th_quantize_act_nhwc_int8

each with an f32 residual and with a codes residual (the composition decodes nothing: it adds an f32 map either way, which favours it).
The yardstick, th_conv2d_q8q8_fwd_affine with its ReLU on the same shape, is timed before and after the new entries in the same run.

Model rows (host library, eager: tensor allocation and launch work included): a three-stage residual model -- stem, two blocks a stage,
exact-stride downsampling with the pointwise projection, global average pool, Linear -- and its bottleneck twin on 28 x 28 inputs at
B = 256 and B = 1: the float model in eval mode, quantize_static_residual(chain=False) and quantize_static_residual(chain=True, links=True).

    python tools/bench_quant_residual.py [--reps 30] [--tag NAME] [--out profiles/quant_residual.json] [--products-only]
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

SHAPES = [(32, 32, 28, 3), (64, 64, 14, 3), (64, 128, 14, 1)]      # c_in, c_out, map side, kernel side (stride 1; pad 1 for 3x3)


class Product:
    """the operands of one static conv and its residual on the device: random codes (the time does not depend on their values)"""

    def __init__(self, ctx, rng, c_in, c_out, side, k, B):
        self.c_in, self.c_out, self.side, self.k, self.B = c_in, c_out, side, k, B
        px = B * side * side
        self.px = px
        self.cpitch, self.cpitch_y = LIB.th_qconv_i8_cpitch(c_in), LIB.th_qconv_i8_cpitch(c_out)
        qx = rng.integers(-128, 128, (px, self.cpitch)).astype(np.int8)
        self.qx, self.ps = ctx.upload(qx.view(np.uint8)), ctx.upload(qx.astype(np.int32).sum(axis=1).astype(np.int32))
        self.qw = ctx.upload(rng.integers(-128, 128, (c_out, k * k, self.cpitch)).astype(np.int8).view(np.uint8))
        self.sx, self.sy, self.sr = (ctx.upload(np.array([v / 127], np.float32)) for v in (4.0, 2.0, 3.0))
        self.wp = ctx.upload(np.stack([np.full(c_out, -0.2, np.float32), np.linspace(1e-3, 2e-3, c_out).astype(np.float32)], axis=1))
        self.ab = ctx.upload(np.stack([np.linspace(0.5, 1.5, c_out).astype(np.float32), np.linspace(-0.1, 0.1, c_out).astype(np.float32)], axis=1))
        self.res = ctx.upload(rng.standard_normal(px * c_out).astype(np.float32))
        self.res_q = ctx.upload(rng.integers(-128, 128, (px, self.cpitch_y)).astype(np.int8).view(np.uint8))
        self.y, self.qy, self.yps = ctx.empty(px * c_out), ctx.empty(px * self.cpitch_y, np.uint8), ctx.empty(px, np.int32)

    def run(self, ctx, kind):
        s, k, pad = self.side, self.k, self.k // 2
        head = (self.qx, self.cpitch, self.ps, self.sx, self.B, self.c_in, s, s, self.qw, self.c_out, k, k, 1, 1, pad, pad, self.wp, None, None)
        codes_tail = (self.sy, self.qy, self.cpitch_y, self.yps, 1, self.ab)
        f32_res, q_res = (self.res, None, 0, None), (None, self.res_q, self.cpitch_y, self.sr)
        n = self.px * self.c_out
        if kind.startswith("yardstick"):
            ctx.call("th_conv2d_q8q8_fwd_affine", *head, 1, self.y, 1, self.ab)
        elif kind.startswith("_residual f32"):
            ctx.call("th_conv2d_q8q8_fwd_residual", *head, 1, self.y, 1, self.ab, *(q_res if "codes residual" in kind else f32_res))
        elif kind.startswith("_codes_residual"):
            ctx.call("th_conv2d_q8q8_fwd_codes_residual", *head, 1, *codes_tail, *(q_res if "codes residual" in kind else f32_res))
        else:      # the composition: the affine product without its ReLU, an f32 add, a ReLU, [the activation codec]
            ctx.call("th_conv2d_q8q8_fwd_affine", *head, 0, self.y, 1, self.ab)
            ctx.call("th_add", self.y, self.res, self.y, n)
            ctx.call("th_relu_fwd", self.y, self.y, n)
            if "codec" in kind:
                ctx.call("th_quantize_act_nhwc_int8", self.y, self.B, self.c_out, s, s, self.sy, self.qy, self.cpitch_y, self.yps)


KINDS = ("yardstick: _affine f32", "_affine + th_add + th_relu_fwd", "_residual f32, f32 residual", "_residual f32, codes residual",
         "_affine + th_add + th_relu_fwd + codec", "_codes_residual, f32 residual", "_codes_residual, codes residual", "yardstick: _affine f32 (again)")


def residual_model(kind, rng):
    """stem -> 2 blocks at 16 channels -> 2 at 32 (the first at stride 2) -> 2 at 64 (the first at stride 2) -> pool -> Linear"""
    if kind == "residual":
        def block(i, o, s, seed): return T.ResidualBlock.pointwise_shortcut(i, o, s, seed=seed)
    else:
        def block(i, o, s, seed): return T.BottleneckBlock(i, max(o // 4, 4), o, s, seed=seed)
    layers = [T.Conv2dReLU(1, 16, (3, 3), None, (1, 1), seed=1)]
    width, seed = 16, 10
    for out, stride in ((16, 1), (32, 2), (64, 2)):
        for b in range(2):
            layers.append(block(width, out, stride if b == 0 else 1, seed))
            width, seed = out, seed + 4
    layers += [T.AdaptiveAvgPool2d((1, 1)), T.Flatten(1), T.Linear(64, 10, True, seed=2)]
    model = T.Sequential(layers)
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
    ap.add_argument("--out", default="profiles/quant_residual.json")
    ap.add_argument("--products-only", action="store_true")
    a = ap.parse_args()
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(r):
        r["build"] = a.tag
        rows.append(r)
        print(json.dumps(r), flush=True)

    for c_in, c_out, side, k in SHAPES:
        p = Product(ctx, rng, c_in, c_out, side, k, 256)
        for kind in KINDS:
            cold, warm = timed(ctx, lambda: p.run(ctx, kind), a.reps, flush)
            report(dict(case=f"product {k}x{k} {c_in}->{c_out} @ {side}x{side}", kind=kind, B=256, cold_us=round(cold, 2), replay_us=round(warm, 2)))
        del p
    if not a.products_only:
        for name in ("residual", "bottleneck"):
            model = residual_model(name, rng)
            calib = T.Tensor(rng.standard_normal((64, 1, 28, 28)).astype(np.float32), (64, 1, 28, 28))
            twins = {"int8 blocks, unchained": model.quantize_static_residual(calib, chain=False),
                     "int8 blocks, chained + links": model.quantize_static_residual(calib, chain=True, links=True)}
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
                outs = {kind: twins[kind](x).data() for kind in twins}
                assert np.array_equal(*(o.view(np.uint32) for o in outs.values())), f"{name} B={B}: the chained twin's output differs from the unchained one's"
                for kind, fn in calls.items():
                    cold, warm = timed_eager(ctx, fn, a.reps, flush)
                    r = dict(case=f"{name} model forward", kind=kind, B=B, cold_us=round(cold, 2), back_to_back_us=round(warm, 2))
                    if kind != "f32 eval":
                        r["err_over_max_abs_float"] = round(float(np.abs(outs[kind] - fl).max() / np.abs(fl).max()), 5)
                        r["chain_links"] = twins[kind].chain_links()
                    report(r)
            del twins, model
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
