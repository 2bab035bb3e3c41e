"""The exact stride-2 3x3 convolution (th_conv3x3_s2_fwd / _bwd_input / _bwd_weight) on MI355X beside what the same library offers without
it, entry points of the parent commit all of them:

  forward          th_conv3x3_fwd (pad 1) on the same input alone -- a composition would still have to subsample its output, so this
                   under-states it -- and th_conv2d_general_fwd with the same geometry (the same arithmetic through an im2col matrix and
                   th_sgemm; its values are quirk Q9's, only its time is used)
  input gradient   th_conv3x3_bwd_input on a gy of the stride-1 shape [n, c_out, h, w]: what a zero-dilated gy would be
  weight gradient  th_conv3x3_bwd_weight on the same gy

Per shape [n, c_in, h, w] -> c_out, us per call replayed back to back between device events (the median of --rounds rounds of --reps
calls).  Every yardstick is timed before and after the new entry, and the new entry is held to the faster of the two.  The forward's
fraction of the 157.3 TFLOP/s fp32 matrix peak counts the strided layer's own products (2 n h_out w_out c_out 9 c_in).

    python tools/bench_strided_conv.py --out profiles/strided_conv.json
    python tools/bench_strided_conv.py --report --out profiles/strided_conv.json      # prints the tables and the verdicts

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
SHAPES = ((256, 32, 28, 28, 64), (256, 64, 14, 14, 128), (256, 16, 28, 28, 32), (64, 4, 9, 9, 8))
PEAK_TFLOPS = 157.3
P, I, F, Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
PROTOS = {
    "th_ctx_create": [I, P], "th_ctx_sync": [P], "th_malloc": [P, Z, P], "th_memcpy_h2d": [P, P, P, Z],
    "th_event_create": [P], "th_event_record": [P, P], "th_event_elapsed_ms": [P, P, P],
    "th_conv3x3_fwd": [P] * 5 + [I] * 8, "th_conv2d_general_fwd": [P] * 5 + [I] * 14,
    "th_conv3x3_bwd_input": [P] * 4 + [I] * 8, "th_conv3x3_bwd_weight": [P] * 4 + [I] * 8,
    "th_conv3x3_s2_fwd": [P] * 5 + [I] * 7, "th_conv3x3_s2_bwd_input": [P] * 4 + [I] * 7, "th_conv3x3_s2_bwd_weight": [P] * 4 + [I] * 7,
}


class Lib:
    def __init__(self, path):
        self.lib = C.CDLL(str(path))
        for name, args in PROTOS.items():
            f = getattr(self.lib, name)
            f.argtypes, f.restype = args, I
        self.lib.th_last_error.restype = C.c_char_p
        h = P()
        self.call("th_ctx_create", 0, C.byref(h), ctx=False)
        self.h = h.value

    def call(self, name, *args, ctx=True):
        rc = getattr(self.lib, name)(*((self.h,) if ctx else ()), *args)
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
        self.call("th_event_create", C.byref(e), ctx=False)
        return e.value

    def timed(self, fn, reps, rounds):
        """-> us per call: the median over `rounds` of `reps` calls back to back between two events"""
        e0, e1, ms, out = self.event(), self.event(), F(), []
        fn()
        self.call("th_ctx_sync")
        for _ in range(rounds):
            self.call("th_event_record", e0)
            for _ in range(reps):
                fn()
            self.call("th_event_record", e1)
            self.call("th_ctx_sync")
            self.call("th_event_elapsed_ms", e0, e1, C.byref(ms), ctx=False)
            out.append(ms.value * 1e3 / reps)
        return round(statistics.median(out), 2)


def measure(L, a):
    rng = np.random.default_rng(0)
    rows = []
    for n, ci, h, w, co in SHAPES:
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        x = L.upload(rng.standard_normal((n, ci, h, w)))
        wt = L.upload(rng.standard_normal((co, ci, 3, 3)) * 0.1)
        bias = L.upload(rng.standard_normal(co))
        gy2 = L.upload(rng.standard_normal((n, co, ho, wo)))      # the strided layer's gy
        gy1 = L.upload(rng.standard_normal((n, co, h, w)))        # the stride-1 shape: what a zero-dilated gy would be
        y1, y2, yg = L.empty(n * co * h * w), L.empty(n * co * ho * wo), L.empty(n * co * ho * wo)
        gx1, gx2, gw1, gw2 = L.empty(n * ci * h * w), L.empty(n * ci * h * w), L.empty(co * ci * 9), L.empty(co * ci * 9)
        t = lambda fn: L.timed(fn, a.reps, a.rounds)
        fwd1 = lambda: L.call("th_conv3x3_fwd", x, wt, bias, y1, n, ci, h, w, co, 1, 0, 1)
        fwdg = lambda: L.call("th_conv2d_general_fwd", x, wt, bias, yg, n, ci, h, w, co, 3, 3, 2, 2, 1, 1, 1, 1, 1)
        fwd2 = lambda: L.call("th_conv3x3_s2_fwd", x, wt, bias, y2, n, ci, h, w, co, 0, 1)
        bwi1 = lambda: L.call("th_conv3x3_bwd_input", gy1, wt, gx1, n, ci, h, w, co, 1, 0, 0)
        bwi2 = lambda: L.call("th_conv3x3_s2_bwd_input", gy2, wt, gx2, n, ci, h, w, co, 0, 0)
        bww1 = lambda: L.call("th_conv3x3_bwd_weight", x, gy1, gw1, n, ci, h, w, co, 1, 0, 0)
        bww2 = lambda: L.call("th_conv3x3_s2_bwd_weight", x, gy2, gw2, n, ci, h, w, co, 0, 0)
        row = dict(tag=a.tag, shape=[n, ci, h, w, co])
        row.update(fwd_s1_first_us=t(fwd1), fwd_general_first_us=t(fwdg), fwd_s2_us=t(fwd2), fwd_s1_again_us=t(fwd1), fwd_general_again_us=t(fwdg))
        row.update(bwd_input_s1_first_us=t(bwi1), bwd_input_s2_us=t(bwi2), bwd_input_s1_again_us=t(bwi1))
        row.update(bwd_weight_s1_first_us=t(bww1), bwd_weight_s2_us=t(bww2), bwd_weight_s1_again_us=t(bww1))
        row["fwd_s2_tflops"] = round(2.0 * n * ho * wo * co * 9 * ci / (row["fwd_s2_us"] * 1e-6) / 1e12, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def report(rows):
    ok = True
    print("| shape [n, c_in, h, w] -> c_out | pass | yardstick | yardstick us (first, again) | stride-2 entry us | entry / faster yardstick | verdict |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        n, ci, h, w, co = r["shape"]
        for key, s2, name, yard in (("fwd_s1", "fwd_s2_us", "forward", "th_conv3x3_fwd alone"), ("fwd_general", "fwd_s2_us", "forward", "th_conv2d_general_fwd"),
                                    ("bwd_input_s1", "bwd_input_s2_us", "input gradient", "th_conv3x3_bwd_input, stride-1 gy"),
                                    ("bwd_weight_s1", "bwd_weight_s2_us", "weight gradient", "th_conv3x3_bwd_weight, stride-1 gy")):
            first, again = r[f"{key}_first_us"], r[f"{key}_again_us"]
            good = r[s2] <= min(first, again)
            ok &= good
            print(f"| [{n}, {ci}, {h}, {w}] -> {co} | {name} | {yard} | {first}, {again} | {r[s2]} | {r[s2] / min(first, again):.2f} | "
                  f"{'not slower' if good else 'SLOWER'} |")
    print()
    print("| shape | forward us | TFLOP/s of the strided layer's products | fraction of the 157.3 TFLOP/s matrix peak |")
    print("|---|---|---|---|")
    for r in rows:
        n, ci, h, w, co = r["shape"]
        print(f"| [{n}, {ci}, {h}, {w}] -> {co} | {r['fwd_s2_us']} | {r['fwd_s2_tflops']} | {r['fwd_s2_tflops'] / PEAK_TFLOPS:.3f} |")
    print()
    print("PASS" if ok else "FAIL")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=str(ROOT / "taper_amd" / "lib" / "libtaper_hip.so"))
    ap.add_argument("--tag", default="new")
    ap.add_argument("--out", default="profiles/strided_conv.json")
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
