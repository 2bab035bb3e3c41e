"""Shared by tests/test_conv_pw_plan.py (no GPU) and tests/test_gpu_conv_pw_forms.py: th_debug_conv1x1_exact_plan as a dict, the sweep that finds
every reachable kernel form of the exact pointwise convolution entry points (csrc/conv_pw.hip), the GPU case table, and the exact reference.

A CASE is (op, n, c_in, h, w, c_out, stride, layout, relu_bias, accumulate, w_off): op 0 th_conv1x1_exact_fwd, 1 _bwd_input, 2 _bwd_weight; h, w
are the INPUT's; relu_bias = relu + 2 * (bias present); w_off: bytes of the weight pointer (op 2: of gw) off a 16-byte boundary.  A FORM is
(op, CT, stride, accumulate (op 1) or the reduce ending (op 2)): which kernel instance runs and which of its paths.  The kernels tile ONE flat
pixel axis (image, oh, ow) in runs of 128, so no row or column is ever split and the plan has no tiling variant to tell apart.

The reference.  A pointwise convolution reads x at [::s, ::s] and is a matrix product over the channels there:
    forward     y  = W . x[:, :, ::s, ::s] (+ bias) (ReLU)
    input_grad  gx[:, :, ::s, ::s] = W^T . gy, +0.0 everywhere else
    weight_grad gw = sum over images and pixels of gy (x) x[:, :, ::s, ::s]
contracted by numpy in float64 (tests/test_conv_pw_plan.py checks all three against torch's conv2d(stride=s) and its autograd, on bits).

Exactness.  x, w and gy are integers in [-4, 4], bias and the initial output (accumulate) integers in [-8, 8]: a forward output or an input
gradient is bounded by 16 * max(c_in, c_out) + 16, a weight gradient by 16 * n * h_out * w_out + 8; every partial sum is an integer below
2^24, so every float32 summation order gives the bits of numpy's float64 result.  A sum that is zero is +0.0: every accumulator starts there."""
import ctypes as C
import functools
import itertools

import numpy as np

f32 = np.float32
PLAN_FIELDS = ("op", "ct", "acc", "stride", "px_t", "span", "tiles", "grid_x", "grid_y", "grid_z", "lds", "lds_limit", "G", "slabs", "reduce",
               "ci_slab", "co_ld", "refused", "h_out", "w_out")
FWD, BWD_INPUT, BWD_WEIGHT = range(3)
OP_NAMES = ("pw_fwd", "pw_bwd_input", "pw_bwd_weight")
KERNEL_NAMES = ("conv_pw_kernel<fwd>", "conv_pw_kernel<bwd>", "conv_pw_wgrad_kernel")
ENTRY_POINTS = ("th_conv1x1_exact_fwd", "th_conv1x1_exact_bwd_input", "th_conv1x1_exact_bwd_weight")
R_NONE, R_SLAB_SUM, R_COLSUM, R_COLSUM_ACCUM, R_SCATTER = range(5)
REDUCE_NAMES = ("none", "slab_sum_kernel", "th_colsum", "th_colsum_accum", "th_colsum + wgrad_scatter_kernel")


def _lib():
    from taper_amd._lib import hip
    return hip


def out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def plan(op, n, c_in, h, w, c_out, stride=1, layout=0, relu_bias=0, acc=0, w_off=0):
    """th_debug_conv1x1_exact_plan as a dict (pure host code: no context, no device)"""
    out = (C.c_int * len(PLAN_FIELDS))()
    assert _lib().th_debug_conv1x1_exact_plan(op, n, c_in, h, w, c_out, stride, layout, relu_bias, acc, w_off, C.cast(out, C.c_void_p)) == 0, \
        _lib().th_last_error()
    return dict(zip(PLAN_FIELDS, out))


def form_from(case, p):
    op = case[0]
    if p["refused"]:
        return (op, 0, p["stride"], p["refused"])
    return (op, p["ct"], p["stride"], (0, p["acc"], p["reduce"])[op])


def form_of(*case):
    return form_from(case, plan(*case))


def form_name(f):
    op, ct, s, v = f
    if ct == 0:
        return f"{OP_NAMES[op]} stride {s}: refused ({v})"
    name = f"{OP_NAMES[op]} stride {s}: {KERNEL_NAMES[op]} CT={ct}"
    if op == BWD_INPUT:
        name += f" accumulate={v}"
    if op == BWD_WEIGHT:
        name += f" {REDUCE_NAMES[v]}"
    return name


def predicted_config(p):
    """what th_debug_last_conv_pw_config reports after a launch of plan p"""
    return [p["op"], p["ct"], p["acc"], p["stride"], p["grid_x"], p["grid_y"], p["grid_z"], p["lds"], p["reduce"]]


# ---------------------------------------------------------------------------------------------------------------- the sweep
SWEEP_C = (1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128)
SWEEP_N = (1, 2, 3, 9, 15, 31, 96, 128, 129, 257, 1536)
# input planes: one pixel, the smallest even side, odd x even, a lone column pair, whole small maps, an image of more than one 128-pixel tile,
# long rows
SWEEP_PLANES = ((1, 1), (2, 2), (5, 6), (6, 5), (7, 2), (8, 8), (33, 20), (14, 14), (28, 28), (3, 255), (3, 300))


def _variants(op):
    """(layout, relu_bias, accumulate, w_off) an op's plan can tell apart"""
    if op == FWD:
        return [(0, 3, 0, 0)]
    if op == BWD_INPUT:
        return [(0, 0, acc, 0) for acc in (0, 1)]
    return [(lay, 0, acc, off) for lay in (0, 1) for acc in (0, 1) for off in (0, 4)]


def _size(c):
    return c[1] * max(c[2], c[5]) * c[3] * c[4]


def exact(c):
    """the case stands inside the exactness argument above"""
    n, c_in, h, w, c_out, s = c[1:7]
    ho, wo = out_hw(h, w, s)
    return 16 * max(c_in, c_out) + 16 < 2 ** 24 and 16 * n * ho * wo + 8 < 2 ** 24


def violations(case, p):
    """what any launch needs of its plan: [] or the broken invariants of plan p of `case`"""
    op, n, c_in, h, w, c_out, s, lay, rb, acc, off = case
    bad = []
    if p["refused"]:
        return bad
    ho, wo = out_hw(h, w, s)
    total = n * ho * wo
    if (p["h_out"], p["w_out"], p["stride"]) != (ho, wo, s):
        bad.append("h_out / w_out / stride")
    if min(p["grid_x"], p["grid_y"], p["grid_z"], p["tiles"]) < 1 or p["grid_x"] >= 2 ** 31 or max(p["grid_y"], p["grid_z"]) > 65535:
        bad.append("a grid dimension below 1 or over the device limit")
    if p["px_t"] != 128 or p["tiles"] != -(-total // 128):
        bad.append("the tiles do not cover the flat pixel axis")
    if not 0 < p["lds"] <= p["lds_limit"] <= 64 << 10:
        bad.append("LDS over the limit of a launch without an attribute")
    if p["ct"] not in (1, 2, 4):
        bad.append("CT")
    if op != BWD_WEIGHT:
        ch, k_ch, src_img = (c_out, c_in, c_in * h * w) if op == FWD else (c_in, c_out, c_out * ho * wo)
        if p["grid_x"] != p["tiles"] or p["grid_y"] != -(-ch // (16 * p["ct"])) or p["grid_z"] != 1:
            bad.append("grid")
        # 128 consecutive pixels that begin at pixel o of an image end in image (o + 127) // P: the worst o is P - 1
        if p["span"] != min(n, (ho * wo - 1 + 127) // (ho * wo) + 1) or p["span"] * src_img * 4 >= 2 ** 31:
            bad.append("the images a tile touches, or their bytes behind one descriptor")
        if p["lds"] != 16 * (16 * p["ct"] + 8) * 4:
            bad.append("LDS of the weight pass")
    else:
        if not 1 <= p["G"] <= min(p["tiles"], 512) or p["slabs"] != p["G"] or p["grid_x"] != p["G"]:
            bad.append("G over min(pixel blocks, 512), or slabs != G")
        if p["ci_slab"] != 32 or p["grid_y"] != -(-c_in // 32) or p["grid_z"] * 16 * p["ct"] != p["co_ld"] or p["co_ld"] < c_out:
            bad.append("slab grid / channel pitch")
        if max(n * c_in * h * w, total * c_out) * 4 >= 2 ** 31:
            bad.append("a map of 2 GiB and more behind one descriptor")
        if p["lds"] != (32 + 16 * p["ct"]) * 130 * 4:
            bad.append("LDS of the two staged operands")
        if p["reduce"] == R_NONE:
            bad.append("slabs without a reduce ending")
        if p["reduce"] == R_SLAB_SUM and not (lay == 0 and off == 0 and p["slabs"] >= 16 and c_in * c_out % 4 == 0 and p["co_ld"] == c_out):
            bad.append("slab_sum_kernel needs 16 slabs, whole quads and an aligned gw in the taper layout")
    return bad


@functools.lru_cache(maxsize=None)
def sweep():
    """one pass over the sweep -> ({form: the smallest exact case that reaches it}, [(case, broken invariant)])"""
    found, bad = {}, []
    for op in range(3):
        var = _variants(op)
        for s, (h, w), c_in, c_out, n in itertools.product((1, 2), SWEEP_PLANES, SWEEP_C, SWEEP_C, SWEEP_N):
            for lay, rb, acc, off in var:
                c = (op, n, c_in, h, w, c_out, s, lay, rb, acc, off)
                if not exact(c):
                    continue
                p = plan(*c)
                f = form_from(c, p)
                if f not in found or _size(c) < _size(found[f]):
                    found[f] = c
                bad += [(c, b) for b in violations(c, p)]
    return found, bad


def reachable_forms():
    return sweep()[0]


# ---------------------------------------------------------------------------------------------------------------- data and reference
def operands(case, seed=0):
    """integer operands as they lie in memory: x [n, c_in, h, w], w [c_out, c_in, 1, 1] (the buffer; layout says how it is read),
    bias [c_out], gy [n, c_out, h_out, w_out]"""
    op, n, c_in, h, w, c_out, s = case[:7]
    rng = np.random.default_rng([seed, 3, op, n, c_in, h, w, c_out, s])
    ho, wo = out_hw(h, w, s)
    x = rng.integers(-4, 5, (n, c_in, h, w), dtype=np.int8).astype(f32)
    wt = rng.integers(-4, 5, (c_out, c_in, 1, 1), dtype=np.int8).astype(f32)
    bias = rng.integers(-8, 9, c_out).astype(f32)
    gy = rng.integers(-4, 5, (n, c_out, ho, wo), dtype=np.int8).astype(f32)
    return x, wt, bias, gy


def initial(case, shape, seed=1):
    """the integer y0 an accumulating call starts from"""
    return np.random.default_rng([seed, 3] + [int(v) & 0xFFFF for v in case[:7]]).integers(-8, 9, shape).astype(f32)


def poison_skipped(x, s):
    """x with NaN in every pixel a stride-s pointwise convolution must not read"""
    xp = np.full_like(x, np.nan)
    xp[:, :, ::s, ::s] = x[:, :, ::s, ::s]
    return xp


def matrix(wt, layout):
    """W[co][ci] float64 of the weight buffer under `layout` (0: the buffer is [c_in][c_out], 1: [c_out][c_in])"""
    c_out, c_in = wt.shape[:2]
    return (wt.reshape(c_in, c_out).T if layout == 0 else wt.reshape(c_out, c_in)).astype(np.float64)


def forward(x, wt, bias, s, layout, relu):
    """[n, c_out, h_out, w_out] float32"""
    xs = x[:, :, ::s, ::s].astype(np.float64)
    y = 0.0 + np.einsum("oc,nchw->nohw", matrix(wt, layout), xs)
    if bias is not None:
        y = y + bias.astype(np.float64)[None, :, None, None]
    if relu:
        y = np.maximum(y, 0.0)
    return np.ascontiguousarray(y.astype(f32))


def input_grad(gy, wt, c_in, h, w, s, layout):
    """[n, c_in, h, w] float32: +0.0 in the pixels no output reads"""
    gx = np.zeros((gy.shape[0], c_in, h, w), np.float64)
    gx[:, :, ::s, ::s] = 0.0 + np.einsum("oc,nohw->nchw", matrix(wt, layout), gy.astype(np.float64))
    return gx.astype(f32)


def weight_grad(x, gy, s, layout):
    """[c_out, c_in, 1, 1] float32 as the gradient lies in memory under `layout`"""
    gw = 0.0 + np.einsum("nohw,nchw->oc", gy.astype(np.float64), x[:, :, ::s, ::s].astype(np.float64))
    mem = gw.T if layout == 0 else gw
    return np.ascontiguousarray(mem).astype(f32).reshape(gw.shape[0], gw.shape[1], 1, 1)


# ---------------------------------------------------------------------------------------------------------------- the GPU case table
def _c(op, n, c_in, h, w, c_out, s=1, layout=0, relu_bias=None, acc=0, w_off=0):
    return (op, n, c_in, h, w, c_out, s, layout, (3 if op == FWD else 0) if relu_bias is None else relu_bias, acc, w_off)


PLANES = ((1, 1), (2, 2), (5, 6), (6, 5), (7, 2), (33, 20))      # even and odd sides (the quad cut by the plane's edge), one image of several tiles
OPS, STRIDES = range(3), (1, 2)
NAMED_CASES = tuple(
    # ---- every plane at both strides, three images (tiles that run over image boundaries), one channel past a 8 and one past a 16-channel
    #      tile, both layouts
    [_c(op, 3, 9, h, w, 17, s, layout=lay) for op in OPS for s in STRIDES for h, w in PLANES for lay in (0, 1)]
    # ---- and the other way round for the input gradient (c_in takes the channel tiles, c_out the passes); 17 is also one past a 16-channel pass
    + [_c(op, 3, 17, h, w, 9, s) for op in OPS for s in STRIDES for h, w in PLANES]
    # ---- channel counts around a k-step (4), 8 and a tile / pass (16), one image
    + [_c(op, 1, ci, 5, 6, co, s) for op in OPS for s in STRIDES for ci in (1, 3, 8, 9) for co in (1, 5, 16, 17)]
    # ---- one past the weight gradient's 32-channel slab
    + [_c(BWD_WEIGHT, 3, 33, 6, 5, 17, s) for s in STRIDES]
    # ---- image counts: one, three, fifteen; 128 one-pixel images fill a tile (its descriptor covers 128 images) and 129 are one past it
    + [_c(op, n, 8, 5, 6, 16, s) for op in OPS for s in STRIDES for n in (1, 3, 15)]
    + [_c(op, n, 3, 1, 1, 5, s) for op in OPS for s in STRIDES for n in (128, 129)]
    # ---- accumulate on both gradients, both layouts, both strides
    + [_c(op, 3, 9, h, w, 17, s, layout=lay, acc=1) for op in (BWD_INPUT, BWD_WEIGHT) for s in STRIDES for h, w in ((6, 5), (33, 20)) for lay in (0, 1)]
    # ---- the four bias x ReLU combinations
    + [_c(FWD, 3, 9, 6, 5, 17, s, relu_bias=rb) for s in STRIDES for rb in range(4)]
    # ---- a weight pointer and a gw pointer 4 bytes past a 16-byte boundary
    + [_c(op, 3, 8, 6, 5, 16, s, w_off=4) for op in (FWD, BWD_INPUT) for s in STRIDES]
    + [_c(BWD_WEIGHT, 3, 8, 6, 5, 16, s, acc=a, w_off=4) for s in STRIDES for a in (0, 1)]
    # ---- long rows (nothing is split: the flat axis runs through them), the last column of an even width
    + [_c(op, 2, 3, 3, 300, 5, s) for op in OPS for s in STRIDES] + [_c(op, 2, 3, 3, 299, 5, 2, layout=1) for op in OPS]
    # ---- the weight gradient's G on both sides of slab_sum_kernel's 16 slabs: 1950 / 1890 pixels (16 / 15 blocks), 1926 / 1917 at stride 2
    + [_c(BWD_WEIGHT, n, 8, 5, 6, 16, 1) for n in (65, 63)] + [_c(BWD_WEIGHT, n, 8, 5, 6, 16, 2) for n in (214, 213)]
)

# the smallest shape of the sweep for every form the named cases above do not reach (regenerate: python -m tests.conv_pw_ref)
GENERATED_CASES = [
    (0, 128, 1, 14, 14, 65, 1, 0, 3, 0, 0),   # pw_fwd stride 1: conv_pw_kernel<fwd> CT=4
    (0, 96, 1, 3, 255, 65, 2, 0, 3, 0, 0),   # pw_fwd stride 2: conv_pw_kernel<fwd> CT=4
    (1, 1, 17, 1, 1, 1, 1, 0, 0, 1, 0),   # pw_bwd_input stride 1: conv_pw_kernel<bwd> CT=2 accumulate=1
    (1, 1, 17, 1, 1, 1, 2, 0, 0, 1, 0),   # pw_bwd_input stride 2: conv_pw_kernel<bwd> CT=2 accumulate=1
    (1, 128, 65, 14, 14, 1, 1, 0, 0, 0, 0),   # pw_bwd_input stride 1: conv_pw_kernel<bwd> CT=4 accumulate=0
    (1, 128, 65, 14, 14, 1, 1, 0, 0, 1, 0),   # pw_bwd_input stride 1: conv_pw_kernel<bwd> CT=4 accumulate=1
    (1, 96, 65, 3, 255, 1, 2, 0, 0, 0, 0),   # pw_bwd_input stride 2: conv_pw_kernel<bwd> CT=4 accumulate=0
    (1, 96, 65, 3, 255, 1, 2, 0, 0, 1, 0),   # pw_bwd_input stride 2: conv_pw_kernel<bwd> CT=4 accumulate=1
    (2, 3, 1, 33, 20, 32, 1, 0, 0, 0, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=2 slab_sum_kernel
    (2, 1, 1, 1, 1, 32, 1, 0, 0, 0, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=2 th_colsum
    (2, 1, 1, 1, 1, 32, 1, 0, 0, 1, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=2 th_colsum_accum
    (2, 9, 1, 3, 255, 32, 2, 0, 0, 0, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=2 slab_sum_kernel
    (2, 1, 1, 1, 1, 32, 2, 0, 0, 0, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=2 th_colsum
    (2, 1, 1, 1, 1, 32, 2, 0, 0, 1, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=2 th_colsum_accum
    (2, 3, 1, 33, 20, 64, 1, 0, 0, 0, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=4 slab_sum_kernel
    (2, 1, 1, 1, 1, 64, 1, 0, 0, 0, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=4 th_colsum
    (2, 1, 1, 1, 1, 64, 1, 0, 0, 1, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=4 th_colsum_accum
    (2, 1, 1, 1, 1, 64, 1, 1, 0, 0, 0),   # pw_bwd_weight stride 1: conv_pw_wgrad_kernel CT=4 th_colsum + wgrad_scatter_kernel
    (2, 9, 1, 3, 255, 64, 2, 0, 0, 0, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=4 slab_sum_kernel
    (2, 1, 1, 1, 1, 64, 2, 0, 0, 0, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=4 th_colsum
    (2, 1, 1, 1, 1, 64, 2, 0, 0, 1, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=4 th_colsum_accum
    (2, 1, 1, 1, 1, 64, 2, 1, 0, 0, 0),   # pw_bwd_weight stride 2: conv_pw_wgrad_kernel CT=4 th_colsum + wgrad_scatter_kernel
]

CASES = list(dict.fromkeys(list(NAMED_CASES) + GENERATED_CASES))


def case_id(c):
    op, n, c_in, h, w, c_out, s, lay, rb, acc, off = c
    return (f"{OP_NAMES[op]}-s{s}-{n}x{c_in}x{h}x{w}-{c_out}-l{lay}" + ("" if rb == (3 if op == FWD else 0) else f"-rb{rb}") +
            ("-acc" if acc else "") + ("-off" if off else ""))


def cases_by_form():
    out = {}
    for c in CASES:
        out.setdefault(form_of(*c), []).append(c)
    return out


if __name__ == "__main__":      # prints what GENERATED_CASES lacks, then the forms
    have, reach = cases_by_form(), reachable_forms()
    for f in sorted(reach):
        if f not in have:
            print(f"    {reach[f]},   # {form_name(f)}")
    print(f"{len(reach)} forms reachable, {len(have)} reached by the case table; per op: " +
          ", ".join(f"{OP_NAMES[op]} {sum(1 for f in reach if f[0] == op)}" for op in range(3)))
    for f in sorted(reach):
        print(f"  {form_name(f)}   e.g. {reach[f]}")
