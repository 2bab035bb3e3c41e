"""The 24 instances of the int8 conv product that predate the residual epilogue (NT 1 / 2 / 4 x f32 / codes destination x one weight pair /
one per channel x plain / affine), timed through the C ABI of ONE kernel library given by path, graph-replayed: run it once per build
(this tree's library, a parent commit's) in processes of their own, alternated, and compare (profiles/quant_residual.md).

The library is loaded by path with nothing else of the project in the process: two builds in one process would share their kernels'
weak symbols, and one of them would be timed twice.

    python tools/bench_qconv_instances.py --lib taper_amd/lib/libtaper_hip.so [--reps 50] [--tag NAME] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
from pathlib import Path

import numpy as np

P, I, F = C.c_void_p, C.c_int, C.c_float
HEAD = [P, P, I, P, P, I, I, I, I, P, I, I, I, I, I, I, I, P, P, P, I]      # ctx .. relu: the 21 every entry point takes
SHAPES = [(32, 28), (64, 14)]      # c_in, map side; B = 256, 3x3, pad 1
C_OUTS = (32, 64, 128)             # NT 1, 2, 4


def load(path):
    lib = C.CDLL(str(path))
    sigs = {"th_ctx_create": [I, P], "th_ctx_destroy": [P], "th_ctx_sync": [P], "th_malloc": [P, C.c_size_t, P], "th_memcpy_h2d": [P, P, P, C.c_size_t],
            "th_event_create": [P], "th_event_record": [P, P], "th_event_elapsed_ms": [P, P, P], "th_graph_begin": [P], "th_graph_end": [P, P],
            "th_graph_launch": [P, P], "th_graph_destroy": [P],
            "th_conv2d_q8q8_fwd": HEAD + [P], "th_conv2d_q8q8_fwd_pc": HEAD + [P], "th_conv2d_q8q8_fwd_affine": HEAD + [P, I, P],
            "th_conv2d_q8q8_fwd_codes": HEAD + [P, P, I, P], "th_conv2d_q8q8_fwd_codes_pc": HEAD + [P, P, I, P],
            "th_conv2d_q8q8_fwd_codes_affine": HEAD + [P, P, I, P, I, P]}
    for name, args in sigs.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = args, I
    lib.th_last_error.restype = C.c_char_p
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--tag", default="this build")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = load(Path(a.lib).resolve())

    def ok(rc):
        if rc != 0:
            raise RuntimeError(lib.th_last_error().decode())

    ctx = P()
    ok(lib.th_ctx_create(0, C.byref(ctx)))

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        d = P()
        ok(lib.th_malloc(ctx, max(arr.nbytes, 4), C.byref(d)))
        ok(lib.th_memcpy_h2d(ctx, d, arr.ctypes.data, arr.nbytes))
        return d

    def event():
        e = P()
        ok(lib.th_event_create(C.byref(e)))
        return e

    e0, e1 = event(), event()
    rng = np.random.default_rng(0)
    rows, B = [], 256
    for c_in, side in SHAPES:
        px = B * side * side
        qx = rng.integers(-128, 128, (px, c_in)).astype(np.int8)      # (c_in is a multiple of 16: the pitch is c_in)
        dqx, dps = upload(qx.view(np.uint8)), upload(qx.astype(np.int32).sum(axis=1).astype(np.int32))
        dsx, dsy, dbp = upload(np.array([4.0 / 127], np.float32)), upload(np.array([2.0 / 127], np.float32)), upload(np.array([-0.1, 0.001], np.float32))
        for c_out in C_OUTS:
            dqw = upload(rng.integers(-128, 128, (c_out, 9, c_in)).astype(np.int8).view(np.uint8))
            dqb = upload(rng.integers(-128, 128, c_out).astype(np.int8).view(np.uint8))
            dwp = upload(np.stack([np.full(c_out, -0.2, np.float32), np.linspace(1e-3, 2e-3, c_out).astype(np.float32)], axis=1))
            dab = upload(np.stack([np.linspace(0.5, 1.5, c_out).astype(np.float32), np.linspace(-0.1, 0.1, c_out).astype(np.float32)], axis=1))
            dy, dqy, dyps = upload(np.zeros(px * c_out, np.float32)), upload(np.zeros(px * c_out, np.uint8)), upload(np.zeros(px, np.int32))
            head = (ctx, dqx, c_in, dps, dsx, B, c_in, side, side, dqw, c_out, 3, 3, 1, 1, 1, 1, dwp, dqb, dbp, 1)
            for codes in (0, 1):
                for pc in (0, 1):
                    for affine in (0, 1):
                        dest = (dsy, dqy, c_out, dyps) if codes else (dy,)
                        if affine:
                            fn, tail = (lib.th_conv2d_q8q8_fwd_codes_affine if codes else lib.th_conv2d_q8q8_fwd_affine), dest + (pc, dab)
                        elif codes:
                            fn, tail = (lib.th_conv2d_q8q8_fwd_codes_pc if pc else lib.th_conv2d_q8q8_fwd_codes), dest
                        else:
                            fn, tail = (lib.th_conv2d_q8q8_fwd_pc if pc else lib.th_conv2d_q8q8_fwd), dest
                        ok(fn(*head, *tail))
                        ok(lib.th_ctx_sync(ctx))
                        ok(lib.th_graph_begin(ctx))
                        ok(fn(*head, *tail))
                        g = P()
                        ok(lib.th_graph_end(ctx, C.byref(g)))
                        ok(lib.th_graph_launch(ctx, g))
                        ok(lib.th_ctx_sync(ctx))
                        ok(lib.th_event_record(ctx, e0))
                        for _ in range(a.reps):
                            ok(lib.th_graph_launch(ctx, g))
                        ok(lib.th_event_record(ctx, e1))
                        ms = F()
                        ok(lib.th_event_elapsed_ms(e0, e1, C.byref(ms)))
                        ok(lib.th_ctx_sync(ctx))
                        lib.th_graph_destroy(g)
                        row = dict(build=a.tag, shape=f"{c_in}->{c_out} @ {side}x{side}", nt=c_out // 32, codes=codes, pc=pc, affine=affine,
                                   replay_us=round(ms.value * 1e3 / a.reps, 2))
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))
    lib.th_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
