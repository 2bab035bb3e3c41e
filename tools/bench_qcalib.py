"""Percentile calibration on MI355X: the histogram pass beside the observers' counting pass of the same run, and the whole
calibrated quantize call beside the min / max one.

Kernel rows, each on a 4096^2 normal tensor, on its ReLU and on [256, 32, 28, 28], at 2 048 bins: th_act_hist_update (one multiply per
element, no edge table) and the yardstick th_obs_hist_count (an arithmetic guess checked against an edge table in LDS) -- 4 bytes per
element both; us per call cold (512 MiB written elsewhere before every timed call; median), per graph replay and per call of calls issued
back to back without a graph, and the share of the 8 TB/s HBM bound.  One row for th_act_scale_from_hist (one workgroup).  The two counting passes are timed alternately, tensor by tensor.

Call rows: Module.quantize_static_calibrated (99.99 %, 2 048 bins) and Module.quantize_static_chain on the reference CNN with four
calibration tensors of 64 images -- host wall time around the call and a device synchronise, median of --calls calls.  Calibration runs
once per deployment: the time is recorded, not tuned.

    python tools/bench_qcalib.py [--reps 50] [--calls 5] [--out profiles/quant_calibration.json]

writes the rows as JSON to --out and the table beside it (same name, .md): the committed summary is profiles/quant_calibration.{json,md}.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import bench  # noqa: E402
import taper_amd as T  # noqa: E402
from taper_amd import hip as H  # noqa: E402

HBM = 8e12
BINS = 2048


def timed(ctx, fn, reps, flush):
    """(median cold us, us per graph replay, us per call of `reps` eager calls issued back to back)"""
    e0, e1 = H.Event(), H.Event()
    fn()
    ctx.sync()
    cold = []
    for _ in range(reps):
        ctx.call("th_fill_f32", flush, 1.0, 128 << 20)   # 512 MiB written elsewhere: the tensor leaves L2 and the Infinity Cache
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
    return statistics.median(cold), replay, eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="profiles/quant_calibration.json")
    a = ap.parse_args()
    ctx = H.Ctx(handle=T.Device.ctx_handle())
    rng = np.random.default_rng(0)
    flush = ctx.empty(128 << 20)
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def kernel_row(kind, case, n, cold, warm, eager, **extra):
        report(kind=kind, case=case, elements=n, bytes_per_element=4, cold_us=round(cold, 2), replay_us=round(warm, 2), back_to_back_us=round(eager, 2),
               cold_bw_share=round(4 * n / (cold * 1e-6) / HBM, 3), replay_bw_share=round(4 * n / (warm * 1e-6) / HBM, 3),
               back_to_back_bw_share=round(4 * n / (eager * 1e-6) / HBM, 3), **extra)

    big = rng.standard_normal((4096, 4096)).astype(np.float32)
    cases = (("4096x4096 normal", big), ("4096x4096 ReLU", np.maximum(big, 0)),
             ("[256, 32, 28, 28]", rng.standard_normal((256, 32, 28, 28)).astype(np.float32)))
    for case, a_np in cases:
        n = a_np.size
        x = ctx.upload(a_np)
        rng3, edges = ctx.empty(3), ctx.empty(BINS + 1)
        ctx.call("th_act_range_update", x, n, 1, rng3, rng3.offset(8))
        ctx.call("th_obs_hist_edges", x, n, BINS, edges)
        for kind, call in ((f"th_act_hist_update {BINS} bins", lambda b: ctx.call("th_act_hist_update", x, n, rng3, BINS, b)),
                           (f"th_obs_hist_count {BINS} bins (yardstick)", lambda b: ctx.call("th_obs_hist_count", x, n, edges, BINS, b))) * 2:   # alternately, twice
            bins = ctx.upload(np.zeros(BINS, np.uint64))
            cold, warm, eager = timed(ctx, lambda: call(bins), a.reps, flush)
            got = ctx.download(bins, BINS, np.uint64)
            assert int(got.sum()) == n * (3 * a.reps + 2), "the timed calls did not count every element"
            kernel_row(kind, case, n, cold, warm, eager, fullest_bin_share=round(int(got.max()) / int(got.sum()), 3))
        bins, stats = ctx.upload(np.zeros(BINS, np.uint64)), ctx.empty(8)
        ctx.call("th_act_hist_update", x, n, rng3, BINS, bins)
        cold, warm, eager = timed(ctx, lambda: ctx.call("th_act_scale_from_hist", bins, BINS, rng3, 999900, rng3.offset(8), stats), a.reps, flush)
        report(kind=f"th_act_scale_from_hist {BINS} bins", case=case, cold_us=round(cold, 2), replay_us=round(warm, 2), back_to_back_us=round(eager, 2))
        del x, bins

    model = bench.build_model(T, "cnn_reference")
    shape = (64, 1, 28, 28)
    calib = [T.Tensor(rng.standard_normal(shape).astype(np.float32), shape) for _ in range(4)]
    for kind, make in (("quantize_static_chain (min / max)", lambda: model.quantize_static_chain(calib)),
                       ("quantize_static_calibrated 99.99 % 2048 bins, chain", lambda: model.quantize_static_calibrated(calib)),
                       ("quantize_static_calibrated 100 % 2048 bins, chain", lambda: model.quantize_static_calibrated(calib, percentile=100))) * 2:
        make()
        T.Device.sync()
        ms = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            q = make()
            T.Device.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        report(kind=kind, case="cnn_reference, 4 x [64, 1, 28, 28]", calls=a.calls, median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3),
               static_layers=len(q.act_scales()), kept=[round(c["kept"] / max(c["total"], 1), 6) for c in q.calibration()])
    same = np.array_equal(model.quantize_static_calibrated(calib, percentile=100).act_scales().view(np.uint32), model.quantize_static_chain(calib).act_scales().view(np.uint32))
    assert same, "percentile = 100 does not reproduce the min / max scales"

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1))
    out.with_suffix(".md").write_text(table(rows, a.reps, a.calls))


def table(rows, reps, calls):
    lines = [f"# Percentile calibration on MI355X (`tools/bench_qcalib.py`, {reps} reps; cold = median after writing 512 MiB elsewhere, "
             "replay = one captured call per graph launch, launches back to back; back to back = the same calls without a graph)", "",
             "A counting pass reads every element once: 4 bytes per element; share = bytes / time / 8 TB/s.  The two passes are timed",
             "alternately on the same tensor, each twice (both rounds are listed).", "",
             "| kernel | case | elements | cold µs | replay µs | back to back µs | cold share | replay share | back to back share | fullest bin |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "elements" in r:
            lines.append(f"| {r['kind']} | {r['case']} | {r['elements']} | {r['cold_us']} | {r['replay_us']} | {r['back_to_back_us']} | {r['cold_bw_share']} | "
                         f"{r['replay_bw_share']} | {r['back_to_back_bw_share']} | {r['fullest_bin_share']} |")
    lines += ["", "| kernel | histogram of | cold µs | replay µs | back to back µs |", "|---|---|---|---|---|"]
    lines += [f"| {r['kind']} | {r['case']} | {r['cold_us']} | {r['replay_us']} | {r['back_to_back_us']} |" for r in rows if "elements" not in r and "cold_us" in r]
    lines += ["", f"The whole call (host wall time around the call and a device synchronise, {calls} calls after one warm-up call; the three",
              "forms alternately, each twice):", "", "| call | case | median ms | min ms | static layers |", "|---|---|---|---|---|"]
    lines += [f"| {r['kind']} | {r['case']} | {r['median_ms']} | {r['min_ms']} | {r['static_layers']} |" for r in rows if "median_ms" in r]
    lines += ["", "Not measured here: kernel time apart from launch gaps (a trace), the passes at other bin counts, models other than the reference CNN."]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
