"""The exact pointwise convolution (th_conv1x1_exact_fwd / _bwd_input / _bwd_weight) on MI355X beside what the same library offers without
it, existing entry points all of them:

  the 3x3 projection it replaces   stride 1: th_conv3x3_fwd / _bwd_input / _bwd_weight (pad 1) on the same maps;
                                   stride 2: th_conv3x3_s2_fwd / _bwd_input / _bwd_weight
  forward, stride 1 only           th_conv1x1_fwd(weight_layout 1): the same product, one th_sgemm launch per image
  informative                      one th_sgemm of [n h_out w_out, c_in] x [c_in, c_out]: the product's price without any layout work

Per shape [n, c_in, h, w] -> c_out and stride, us per call: every call is captured `--reps` times into one graph, and the graph is replayed
between two device events (the median of --rounds replays, one warm-up replay in front).  Every yardstick is timed before and after the new
entry, and the new entry is held to the faster of the two.  The forward's products are 2 n h_out w_out c_in c_out (against the 157.3 TFLOP/s
fp32 matrix peak) and its least traffic 4 n h_out w_out (c_in + c_out) bytes (against 8 TB/s); the larger of the two times is the bound.

    python tools/bench_pointwise_conv.py --out profiles/pointwise_conv.json
    python tools/bench_pointwise_conv.py --report --out profiles/pointwise_conv.json      # prints the tables and the verdicts

Loads the kernel library directly (ctypes): nothing of the Python package runs.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((256, 32, 28, 28, 64), (256, 64, 14, 14, 128), (256, 64, 14, 14, 256), (64, 4, 9, 9, 8))
PEAK_TFLOPS, PEAK_TBS = 157.3, 8.0
P, I, F, Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
PROTOS = {
    "th_ctx_create": [I, P], "th_ctx_sync": [P], "th_malloc": [P, Z, P], "th_memcpy_h2d": [P, P, P, Z],
    "th_event_create": [P], "th_event_record": [P, P], "th_event_elapsed_ms": [P, P, P],
    "th_graph_begin": [P], "th_graph_end": [P, P], "th_graph_launch": [P, P], "th_graph_destroy": [P],
    "th_conv3x3_fwd": [P] * 5 + [I] * 8, "th_conv3x3_bwd_input": [P] * 4 + [I] * 8, "th_conv3x3_bwd_weight": [P] * 4 + [I] * 8,
    "th_conv3x3_s2_fwd": [P] * 5 + [I] * 7, "th_conv3x3_s2_bwd_input": [P] * 4 + [I] * 7, "th_conv3x3_s2_bwd_weight": [P] * 4 + [I] * 7,
    "th_conv1x1_fwd": [P] * 5 + [I] * 7, "th_sgemm": [P, I, I, I, I, I, F, P, P, F, P],
    "th_conv1x1_exact_fwd": [P] * 5 + [I] * 8, "th_conv1x1_exact_bwd_input": [P] * 4 + [I] * 8, "th_conv1x1_exact_bwd_weight": [P] * 4 + [I] * 8,
}
NO_CTX = ("th_ctx_create", "th_event_create", "th_event_elapsed_ms", "th_graph_destroy")


class Lib:
    def __init__(self, path):
        self.lib = C.CDLL(str(path))
        for name, args in PROTOS.items():
            f = getattr(self.lib, name)
            f.argtypes, f.restype = args, I
        self.lib.th_last_error.restype = C.c_char_p
        h = P()
        self.call("th_ctx_create", 0, C.byref(h))
        self.h = h.value

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*(() if name in NO_CTX else (self.h,)), *args)
        if rc != 0:
            raise RuntimeError(f"{name}: {self.lib.th_last_error().decode()}")

    def empty(self, n):
        p = P()
        self.call("th_malloc", int(n) * 4, C.byref(p))
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a, np.float32)
        p = self.empty(a.size)
        self.call("th_memcpy_h2d", p, a.ctypes.data, a.nbytes)
        return p

    def event(self):
        e = P()
        self.call("th_event_create", C.byref(e))
        return e.value

    def timed(self, fn, reps, rounds):
        """-> us per call: `reps` calls captured into one graph, the median over `rounds` replays between two events"""
        e0, e1, ms, out, g = self.event(), self.event(), F(), [], P()
        fn()                                   # (code objects loaded, the pool holds the call's workspace before the capture)
        self.call("th_ctx_sync")
        self.call("th_graph_begin")
        for _ in range(reps):
            fn()
        self.call("th_graph_end", C.byref(g))
        self.call("th_graph_launch", g.value)
        self.call("th_ctx_sync")
        for _ in range(rounds):
            self.call("th_event_record", e0)
            self.call("th_graph_launch", g.value)
            self.call("th_event_record", e1)
            self.call("th_ctx_sync")
            self.call("th_event_elapsed_ms", e0, e1, C.byref(ms))
            out.append(ms.value * 1e3 / reps)
        self.call("th_graph_destroy", g.value)
        return round(statistics.median(out), 2)


def measure(L, a):
    rng = np.random.default_rng(0)
    rows = []
    for s in (1, 2):
        for n, ci, h, w, co in SHAPES:
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            px = n * ho * wo
            x = L.upload(rng.standard_normal((n, ci, h, w)))
            w1 = L.upload(rng.standard_normal((co, ci)) * 0.1)
            w3 = L.upload(rng.standard_normal((co, ci, 3, 3)) * 0.1)
            bias = L.upload(rng.standard_normal(co))
            gy = L.upload(rng.standard_normal((n, co, ho, wo)))
            y1, y3, yq, ys = L.empty(px * co), L.empty(px * co), L.empty(px * co), L.empty(px * co)
            gx1, gx3, gw1, gw3 = L.empty(n * ci * h * w), L.empty(n * ci * h * w), L.empty(co * ci), L.empty(co * ci * 9)
            t = lambda fn: L.timed(fn, a.reps, a.rounds)
            if s == 1:
                f3 = lambda: L.call("th_conv3x3_fwd", x, w3, bias, y3, n, ci, h, w, co, 1, 0, 1)
                i3 = lambda: L.call("th_conv3x3_bwd_input", gy, w3, gx3, n, ci, h, w, co, 1, 0, 0)
                g3 = lambda: L.call("th_conv3x3_bwd_weight", x, gy, gw3, n, ci, h, w, co, 1, 0, 0)
            else:
                f3 = lambda: L.call("th_conv3x3_s2_fwd", x, w3, bias, y3, n, ci, h, w, co, 0, 1)
                i3 = lambda: L.call("th_conv3x3_s2_bwd_input", gy, w3, gx3, n, ci, h, w, co, 0, 0)
                g3 = lambda: L.call("th_conv3x3_s2_bwd_weight", x, gy, gw3, n, ci, h, w, co, 0, 0)
            fq = lambda: L.call("th_conv1x1_fwd", x, w1, bias, yq, n, ci, h, w, co, 1, 1)
            fs = lambda: L.call("th_sgemm", 0, 0, px, co, ci, 1.0, x, w1, 0.0, ys)
            f1 = lambda: L.call("th_conv1x1_exact_fwd", x, w1, bias, y1, n, ci, h, w, co, s, 0, 1)
            i1 = lambda: L.call("th_conv1x1_exact_bwd_input", gy, w1, gx1, n, ci, h, w, co, s, 0, 0)
            g1 = lambda: L.call("th_conv1x1_exact_bwd_weight", x, gy, gw1, n, ci, h, w, co, s, 0, 0)
            row = dict(tag=a.tag, stride=s, shape=[n, ci, h, w, co])
            row.update(fwd_3x3_first_us=t(f3), fwd_sgemm_first_us=t(fs))
            if s == 1:
                row.update(fwd_1x1_first_us=t(fq))
            row.update(fwd_pw_us=t(f1), fwd_3x3_again_us=t(f3), fwd_sgemm_again_us=t(fs))
            if s == 1:
                row.update(fwd_1x1_again_us=t(fq))
            row.update(bwd_input_3x3_first_us=t(i3), bwd_input_pw_us=t(i1), bwd_input_3x3_again_us=t(i3))
            row.update(bwd_weight_3x3_first_us=t(g3), bwd_weight_pw_us=t(g1), bwd_weight_3x3_again_us=t(g3))
            row["fwd_flop"] = 2.0 * px * ci * co
            row["fwd_bytes"] = 4.0 * px * (ci + co)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def report(rows):
    ok = True
    print("| stride | shape [n, c_in, h, w] -> c_out | pass | yardstick | yardstick us (first, again) | pointwise entry us | entry / faster yardstick | verdict |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        n, ci, h, w, co = r["shape"]
        s = r["stride"]
        three = "th_conv3x3_" if s == 1 else "th_conv3x3_s2_"
        table = [("fwd_3x3", "fwd_pw_us", "forward", three + "fwd", True), ("bwd_input_3x3", "bwd_input_pw_us", "input gradient", three + "bwd_input", True),
                 ("bwd_weight_3x3", "bwd_weight_pw_us", "weight gradient", three + "bwd_weight", True),
                 ("fwd_sgemm", "fwd_pw_us", "forward", "one th_sgemm (informative)", False)]
        if s == 1:
            table.insert(1, ("fwd_1x1", "fwd_pw_us", "forward", "th_conv1x1_fwd(layout 1)", True))
        for key, pw, name, yard, binding in table:
            first, again = r[f"{key}_first_us"], r[f"{key}_again_us"]
            good = r[pw] <= min(first, again)
            ok &= good or not binding
            verdict = ("not slower" if good else "SLOWER") if binding else "-"
            print(f"| {s} | [{n}, {ci}, {h}, {w}] -> {co} | {name} | {yard} | {first}, {again} | {r[pw]} | {r[pw] / min(first, again):.2f} | {verdict} |")
    print()
    print("| stride | shape | forward us | TFLOP/s | of the 157.3 TFLOP/s matrix peak | GB/s of the least traffic | of 8 TB/s | least time us (bound) | least / measured |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        n, ci, h, w, co = r["shape"]
        us = r["fwd_pw_us"]
        tf, tb = r["fwd_flop"] / (us * 1e-6) / 1e12, r["fwd_bytes"] / (us * 1e-6) / 1e12
        t_f, t_b = r["fwd_flop"] / (PEAK_TFLOPS * 1e12) * 1e6, r["fwd_bytes"] / (PEAK_TBS * 1e12) * 1e6
        print(f"| {r['stride']} | [{n}, {ci}, {h}, {w}] -> {co} | {us} | {tf:.2f} | {tf / PEAK_TFLOPS:.3f} | {tb * 1e3:.0f} | {tb / PEAK_TBS:.3f} | "
              f"{max(t_f, t_b):.2f} ({'matrix' if t_f >= t_b else 'bytes'}) | {max(t_f, t_b) / us:.3f} |")
    print()
    print("PASS" if ok else "FAIL")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=str(ROOT / "taper_amd" / "lib" / "libtaper_hip.so"))
    ap.add_argument("--tag", default="new")
    ap.add_argument("--out", default="profiles/pointwise_conv.json")
    ap.add_argument("--report", action="store_true")
    a = ap.parse_args()
    out = Path(a.out)
    rows = json.loads(out.read_text()) if out.exists() else []
    if a.report:
        raise SystemExit(0 if report(rows) else 1)
    rows += measure(Lib(a.lib), a)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
