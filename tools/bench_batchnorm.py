"""BatchNorm2d's kernels on MI355X beside two yardsticks timed in the same run on a tensor of the same element count.

Per shape [n, c, h, w]: the training forward (th_batchnorm2d_fwd: x read twice, y written -- 12 B per element), the backward
(th_batchnorm2d_bwd with gx: gy and x read twice, gx written -- 20 B) and the eval forward (8 B); th_fake_quant_act(int8), which has the
training forward's traffic (12 B over two passes), and a later th_obs_minmax_update, which moves 20 B like the backward.  Each: us per
call cold (a 512 MiB buffer written elsewhere before every timed call; median) and replayed (back to back), the byte bound at 8 TB/s and
the share of it.  Every yardstick is timed twice in the run: the difference of the two is the spread a kernel is judged within.

    python tools/bench_batchnorm.py [--reps 50] [--out profiles/batchnorm.json]

writes the rows as JSON to --out and the table beside it (same name, .md): the committed summary is profiles/batchnorm.{json,md}.
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
from taper_amd import hip as H  # noqa: E402
from taper_amd._lib import hip as L  # noqa: E402

HBM = 8e12
SHAPES = ((256, 32, 28, 28), (256, 64, 14, 14), (4096, 128, 1, 1), (64, 4, 7, 7))


def timed(ctx, fn, reps, flush):
    e0, e1 = H.Event(), H.Event()
    fn()
    ctx.sync()
    cold = []
    for _ in range(reps):
        ctx.call("th_fill_f32", flush, 1.0, 128 << 20)
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.sync()
        cold.append(ctx.elapsed_ms(e0, e1) * 1e3)
    ctx.record(e0)
    for _ in range(reps):
        fn()
    ctx.record(e1)
    ctx.sync()
    return statistics.median(cold), ctx.elapsed_ms(e0, e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="profiles/batchnorm.json")
    a = ap.parse_args()
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(kind, shape, n, per, launches, cold, warm):
        bound = per * n / HBM * 1e6
        r = dict(kind=kind, shape=list(shape), elements=n, bytes_per_element=per, launches=launches, byte_bound_us=round(bound, 2),
                 cold_us=round(cold, 2), replay_us=round(warm, 2), cold_share_of_bound=round(bound / cold, 3),
                 replay_share_of_bound=round(bound / warm, 3))
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for shape in SHAPES:
        n_, c, h, w = shape
        n, hw = n_ * c * h * w, h * w
        split = L.th_batchnorm2d_split(n_, c, hw)
        x, gy = ctx.upload(rng.standard_normal(shape).astype(np.float32)), ctx.upload((rng.standard_normal(shape) + 0.5).astype(np.float32))
        y, gx, s = ctx.empty(n), ctx.empty(n), ctx.empty(1)
        gamma, beta, rm, rv = ctx.upload(np.ones(c, np.float32)), ctx.zeros(c), ctx.zeros(c), ctx.upload(np.ones(c, np.float32))
        sm, si, gg, gb = ctx.empty(c), ctx.empty(c), ctx.empty(c), ctx.empty(c)
        mn, mx = ctx.empty(n), ctx.empty(n)
        ctx.call("th_obs_minmax_first", x, mn, mx, n)

        def fq():
            ctx.call("th_fake_quant_act", x, y, n, 0, s)

        def mm():
            ctx.call("th_obs_minmax_update", gy, mn, mx, n)

        def fwd_train():
            ctx.call("th_batchnorm2d_fwd", x, gamma, beta, y, rm, rv, sm, si, n_, c, hw, 1e-5, 0.1, 1, 0)

        def fwd_eval():
            ctx.call("th_batchnorm2d_fwd", x, gamma, beta, y, rm, rv, sm, si, n_, c, hw, 1e-5, 0.1, 0, 0)

        def bwd():
            ctx.call("th_batchnorm2d_bwd", gy, x, None, gamma, sm, si, gx, gg, gb, n_, c, hw, 1, 0)

        two = 1 if split == 1 else 2
        report("th_fake_quant_act int8 (yardstick, first)", shape, n, 12, 2, *timed(ctx, fq, a.reps, flush))
        report("th_batchnorm2d_fwd training", shape, n, 12, two, *timed(ctx, fwd_train, a.reps, flush))
        report("th_fake_quant_act int8 (yardstick, again)", shape, n, 12, 2, *timed(ctx, fq, a.reps, flush))
        report("th_obs_minmax_update (yardstick, first)", shape, n, 20, 1, *timed(ctx, mm, a.reps, flush))
        report("th_batchnorm2d_bwd with gx", shape, n, 20, two, *timed(ctx, bwd, a.reps, flush))
        report("th_obs_minmax_update (yardstick, again)", shape, n, 20, 1, *timed(ctx, mm, a.reps, flush))
        report("th_batchnorm2d_fwd eval", shape, n, 8, 1, *timed(ctx, fwd_eval, a.reps, flush))
        rows[-1]["split"] = split
        del x, gy, y, gx, mn, mx

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1) + "\n")
    lines = ["# BatchNorm2d kernels beside their yardsticks (tools/bench_batchnorm.py)", "",
             "us per call: cold (a 512 MiB buffer written before every timed call; median) and replayed back to back; bound = bytes at 8 TB/s.",
             "", "| kernel | shape | launches | B / element | bound us | cold us | replay us | cold share | replay share |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['kind']} | {r['shape']} | {r['launches']} | {r['bytes_per_element']} | {r['byte_bound_us']} | {r['cold_us']} | "
                     f"{r['replay_us']} | {r['cold_share_of_bound']} | {r['replay_share_of_bound']} |")
    out.with_suffix(".md").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
