"""The residual tail's kernels on MI355X beside the composition a user writes without them, and the plain batch-norm calls of two builds.

Per shape [n, c, h, w], us per call replayed back to back between device events (the median of --rounds rounds of --reps calls):

  forward (training)   th_bn_residual_fwd with the ReLU             against   th_batchnorm2d_fwd (relu = 0), th_add, th_relu_fwd
  backward             th_bn_residual_bwd with y (the ReLU's mask)   against   th_relu_bwd, two th_memcpy_d2d (the add's backward into two
                                                                              empty slots), th_batchnorm2d_bwd

The composition is timed before and after the fused entry; the fused entry is held to the faster of the two.  The plain
th_batchnorm2d_fwd / th_batchnorm2d_bwd are timed as well, through whichever libtaper_hip.so --lib names: run once per build (a build
of the parent commit and this build, three runs each, interleaved, for the run-to-run spread) with the same --out, then --report.

    python tools/bench_residual.py --tag new --out profiles/residual.json                 # fused against composition, and plain
    python tools/bench_residual.py --plain --lib <parent build>/libtaper_hip.so --tag parent --out profiles/residual.json
    python tools/bench_residual.py --report --out profiles/residual.json                  # prints the tables and the verdicts

Loads the kernel library directly (ctypes): nothing of the Python package runs, so a library of another commit can stand in.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((256, 32, 28, 28), (256, 64, 14, 14), (4096, 128, 1, 1), (64, 4, 7, 7))
P, I, F, Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
PROTOS = {
    "th_ctx_create": [I, P], "th_ctx_sync": [P], "th_malloc": [P, Z, P], "th_memcpy_h2d": [P, P, P, Z], "th_memcpy_d2d": [P, P, P, Z],
    "th_fill_f32": [P, P, F, Z], "th_event_create": [P], "th_event_record": [P, P], "th_event_elapsed_ms": [P, P, P],
    "th_add": [P, P, P, P, Z], "th_relu_fwd": [P, P, P, Z], "th_relu_bwd": [P, P, P, P, Z, I], "th_batchnorm2d_split": [I, I, I],
    "th_batchnorm2d_fwd": [P] * 9 + [I, I, I, F, F, I, I], "th_batchnorm2d_bwd": [P] * 10 + [I] * 5,
    "th_bn_residual_fwd": [P] * 10 + [I, I, I, F, F, I, I], "th_bn_residual_bwd": [P] * 11 + [I] * 5,
}


class Lib:
    def __init__(self, path, plain):
        self.lib = C.CDLL(str(path))
        for name, args in PROTOS.items():
            if plain and name.startswith("th_bn_residual"):
                continue
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


def measure(L, a, plain):
    rng = np.random.default_rng(0)
    rows = []
    for shape in SHAPES:
        n_, c, h, w = shape
        n, hw = n_ * c * h * w, h * w
        x, r, gy = (L.upload(rng.standard_normal(shape) + b) for b in (0.0, 0.0, 0.5))
        y0, s, y, gs, gh, gx, gr = (L.empty(n) for _ in range(7))
        gamma, beta, rm, rv = L.upload(np.ones(c)), L.upload(np.zeros(c)), L.upload(np.zeros(c)), L.upload(np.ones(c))
        sm, si, gg, gb = (L.empty(c) for _ in range(4))
        t = lambda fn: L.timed(fn, a.reps, a.rounds)

        def plain_fwd():
            L.call("th_batchnorm2d_fwd", x, gamma, beta, y0, rm, rv, sm, si, n_, c, hw, 1e-5, 0.1, 1, 0)

        def plain_bwd():
            L.call("th_batchnorm2d_bwd", gh, x, None, gamma, sm, si, gx, gg, gb, n_, c, hw, 1, 0)

        def comp_fwd():
            plain_fwd()
            L.call("th_add", y0, r, s, n)
            L.call("th_relu_fwd", s, y, n)

        def comp_bwd():
            L.call("th_relu_bwd", s, gy, gs, n, 0)
            L.call("th_memcpy_d2d", gh, gs, n * 4)
            L.call("th_memcpy_d2d", gr, gs, n * 4)
            plain_bwd()

        def fused_fwd():
            L.call("th_bn_residual_fwd", x, r, gamma, beta, y, rm, rv, sm, si, n_, c, hw, 1e-5, 0.1, 1, 1)

        def fused_bwd():
            L.call("th_bn_residual_bwd", gy, x, y, gamma, sm, si, gx, gr, gg, gb, n_, c, hw, 1, 0)

        comp_fwd()      # (s, y and the saved pair hold what the backward passes read)
        L.call("th_memcpy_d2d", gh, gy, n * 4)
        row = dict(tag=a.tag, shape=list(shape), split=L.lib.th_batchnorm2d_split(n_, c, hw), plain_fwd_us=t(plain_fwd), plain_bwd_us=t(plain_bwd))
        if not plain:
            row.update(comp_fwd_first_us=t(comp_fwd), fused_fwd_us=t(fused_fwd), comp_fwd_again_us=t(comp_fwd),
                       comp_bwd_first_us=t(comp_bwd), fused_bwd_us=t(fused_bwd), comp_bwd_again_us=t(comp_bwd))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def report(rows):
    ok = True
    print("| shape | split | pass | composition us (first, again) | fused us | fused / faster composition | verdict |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if "fused_fwd_us" not in r:
            continue
        for k, name in (("fwd", "forward, training"), ("bwd", "backward")):
            comp = min(r[f"comp_{k}_first_us"], r[f"comp_{k}_again_us"])
            good = r[f"fused_{k}_us"] <= comp
            ok &= good
            print(f"| {r['shape']} | {r['split']} | {name} | {r[f'comp_{k}_first_us']}, {r[f'comp_{k}_again_us']} | {r[f'fused_{k}_us']} | "
                  f"{r[f'fused_{k}_us'] / comp:.2f} | {'not slower' if good else 'SLOWER'} |")
    print()
    print("| shape | pass | parent build us (each run) | this build us (each run) | verdict |")
    print("|---|---|---|---|---|")
    for shape in SHAPES:
        for k, name in (("fwd", "th_batchnorm2d_fwd, training"), ("bwd", "th_batchnorm2d_bwd with gx")):
            par = [r[f"plain_{k}_us"] for r in rows if r["shape"] == list(shape) and r["tag"] == "parent"]
            new = [r[f"plain_{k}_us"] for r in rows if r["shape"] == list(shape) and r["tag"] != "parent"]
            if not par or not new:
                continue
            # inside the parent's run-to-run spread: this build's median run is no slower than the parent's slowest run
            good = statistics.median(new) <= max(par)
            ok &= good
            print(f"| {list(shape)} | {name} | {', '.join(map(str, par))} | {', '.join(map(str, new))} | "
                  f"{'inside the spread' if good else 'OUTSIDE'} |")
    print()
    print("PASS" if ok else "FAIL")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lib", default=str(ROOT / "taper_amd" / "lib" / "libtaper_hip.so"))
    ap.add_argument("--plain", action="store_true", help="only th_batchnorm2d_fwd / _bwd (a library without the residual entries)")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--out", default="profiles/residual.json")
    ap.add_argument("--report", action="store_true")
    a = ap.parse_args()
    out = Path(a.out)
    rows = json.loads(out.read_text()) if out.exists() else []
    if a.report:
        raise SystemExit(0 if report(rows) else 1)
    rows += measure(Lib(a.lib, a.plain), a, a.plain)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
