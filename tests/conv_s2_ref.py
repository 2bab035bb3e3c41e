"""Shared by tests/test_conv_s2_plan.py (no GPU) and tests/test_gpu_conv_s2_forms.py: th_debug_conv3x3_s2_plan as a dict, the sweep that finds
every reachable kernel form of the stride-2 3x3 convolution entry points (csrc/conv_s2.hip), the GPU case table, and the exact reference,
written on top of tests/conv_ref.py.

A CASE is (op, n, c_in, h, w, c_out, layout, relu_bias, accumulate, w_off): op 0 th_conv3x3_s2_fwd, 1 _bwd_input, 2 _bwd_weight; h, w are the
INPUT's; relu_bias = relu + 2 * (bias present); w_off: bytes of the weight pointer (op 2: of gw) off a 16-byte boundary.  A FORM is
(op, CT, accumulate (op 1) or the reduce ending (op 2), 1 if a row is cut into column blocks): which kernel instance runs and which of its paths.

The reference.  A stride-2 convolution is the stride-1 convolution read at every second pixel, and its gradients are the stride-1 gradients of
gy put back at every second pixel of a zero map ("dilated"):
    forward     = conv_ref.forward(x, wt, bias, 1, layout, relu)[:, :, ::2, ::2]
    input_grad  = conv_ref.input_grad(dilate(gy), wt, c_in, layout)
    weight_grad = conv_ref.weight_grad(x, dilate(gy), 1, layout)
(tests/test_conv_s2_plan.py checks all three against torch's conv2d(stride=2, padding=1) and its autograd, on bits.)

Exactness.  x, w and gy are integers in [-4, 4], bias and the initial output (accumulate) integers in [-8, 8]: a forward output or an input
gradient is bounded by 16 * 9 * max(c_in, c_out) + 16, a weight gradient by 16 * n * h_out * w_out + 8; every partial sum is an integer below
2^24, so every float32 summation order gives the bits of numpy's float64 result."""
import ctypes as C
import functools
import itertools

import numpy as np

from tests import conv_ref

f32 = np.float32
PLAN_FIELDS = ("op", "ct", "acc", "img_t", "rows_t", "cols_t", "bands", "cblks", "grid_x", "grid_y", "grid_z", "lds", "lds_limit", "G", "slabs",
               "reduce", "n_pb", "co_ld", "refused", "h_out", "w_out")
FWD, BWD_INPUT, BWD_WEIGHT = range(3)
OP_NAMES = ("s2_fwd", "s2_bwd_input", "s2_bwd_weight")
KERNEL_NAMES = ("conv3x3_s2_fwd_kernel", "conv3x3_s2_bwd_input_kernel", "conv3x3_s2_wgrad_kernel")
ENTRY_POINTS = ("th_conv3x3_s2_fwd", "th_conv3x3_s2_bwd_input", "th_conv3x3_s2_bwd_weight")
R_NONE, R_SLAB_SUM, R_COLSUM, R_COLSUM_ACCUM, R_SCATTER = range(5)
REDUCE_NAMES = conv_ref.REDUCE_NAMES


def _lib():
    from taper_amd._lib import hip
    return hip


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def plan(op, n, c_in, h, w, c_out, layout=0, relu_bias=0, acc=0, w_off=0):
    """th_debug_conv3x3_s2_plan as a dict (pure host code: no context, no device)"""
    out = (C.c_int * len(PLAN_FIELDS))()
    assert _lib().th_debug_conv3x3_s2_plan(op, n, c_in, h, w, c_out, layout, relu_bias, acc, w_off, C.cast(out, C.c_void_p)) == 0, \
        _lib().th_last_error()
    return dict(zip(PLAN_FIELDS, out))


def form_from(case, p):
    op = case[0]
    if p["refused"]:
        return (op, 0, p["refused"], 0)
    return (op, p["ct"], (0, p["acc"], p["reduce"])[op], int(p["cblks"] > 1))


def form_of(*case):
    return form_from(case, plan(*case))


def form_name(f):
    op, ct, v, cb = f
    if ct == 0:
        return f"{OP_NAMES[op]}: refused ({v})"
    s = f"{OP_NAMES[op]}: {KERNEL_NAMES[op]}<CT={ct}>"
    if op == BWD_INPUT:
        s += f" accumulate={v}"
    if op == BWD_WEIGHT:
        s += f" {REDUCE_NAMES[v]}"
    return s + (" column blocks" if cb else "")


def predicted_config(p):
    """what th_debug_last_conv_s2_config reports after a launch of plan p"""
    return [p["op"], p["ct"], p["acc"], p["grid_x"], p["grid_y"], p["grid_z"], p["lds"], p["reduce"]]


# ---------------------------------------------------------------------------------------------------------------- the sweep
SWEEP_C = (1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128)
SWEEP_N = (1, 2, 3, 9, 15, 31, 96, 128, 129, 257, 1536)
# input planes: one pixel, the smallest even side, odd x even, a lone column pair, two row bands with a ragged last one, whole small maps,
# the widest row of one column block (w_out = 128) and rows cut into column blocks (w_out = 150)
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
    n, c_in, h, w, c_out = c[1:6]
    ho, wo = out_hw(h, w)
    return 16 * 9 * max(c_in, c_out) + 16 < 2 ** 24 and 16 * n * ho * wo + 8 < 2 ** 24


def violations(case, p):
    """what any launch needs of its plan: [] or the broken invariants of plan p of `case`"""
    op, n, c_in, h, w, c_out, lay, rb, acc, off = case
    bad = []
    if p["refused"]:
        return bad
    ho, wo = out_hw(h, w)
    if (p["h_out"], p["w_out"]) != (ho, wo):
        bad.append("h_out / w_out")
    if min(p["img_t"], p["rows_t"], p["cols_t"], p["grid_x"], p["grid_y"], p["grid_z"]) < 1:
        bad.append("a tile or grid dimension below 1")
    if p["img_t"] * p["rows_t"] * p["cols_t"] > 128:
        bad.append("over 128 pixels per workgroup")
    if p["bands"] != -(-ho // p["rows_t"]) or p["cblks"] != -(-wo // p["cols_t"]) or p["img_t"] > n:
        bad.append("bands / column blocks do not tile the output, or more images per tile than the batch has")
    if not 0 < p["lds"] <= p["lds_limit"] <= 160 << 10:
        bad.append("LDS over the limit the launch requests")
    if p["ct"] not in (1, 2, 4):
        bad.append("CT")
    tiles = -(-n // p["img_t"]) * p["bands"] * p["cblks"]
    if op != BWD_WEIGHT:
        ch = c_out if op == FWD else c_in
        if p["grid_x"] != tiles or p["grid_y"] != -(-ch // (16 * p["ct"])) or p["grid_z"] != 1:
            bad.append("grid")
        chunk = p["img_t"] * ((2 * p["rows_t"] + 1) * (2 * p["cols_t"] + 1) if op == FWD else (p["rows_t"] + 1) * (p["cols_t"] + 1))
        if chunk > (1024 if op == FWD else 512):
            bad.append("a channel's staged chunk over what the threads hold")
    else:
        if p["n_pb"] != tiles or not 1 <= p["G"] <= min(p["n_pb"], 512) or p["slabs"] != p["G"] or p["grid_x"] != p["G"]:
            bad.append("G over min(n_pb, 512), or slabs != G")
        if p["grid_y"] != -(-c_in // 16) or p["grid_z"] * 16 * p["ct"] != p["co_ld"] or p["co_ld"] < c_out:
            bad.append("slab grid / channel pitch")
        if p["img_t"] * (2 * p["rows_t"] + 1) * (2 * p["cols_t"] + 1) > 512:
            bad.append("a channel's staged chunk over 512 floats")
        if p["reduce"] == R_NONE:
            bad.append("slabs without a reduce ending")
        if p["reduce"] == R_SLAB_SUM and not (lay == 0 and off == 0 and p["slabs"] >= 16 and 9 * c_in * c_out % 4 == 0 and p["co_ld"] == c_out):
            bad.append("slab_sum_kernel needs 16 slabs, whole quads and an aligned gw in the taper layout")
    return bad


@functools.lru_cache(maxsize=None)
def sweep():
    """one pass over the sweep -> ({form: the smallest exact case that reaches it}, [(case, broken invariant)])"""
    found, bad = {}, []
    for op in range(3):
        var = _variants(op)
        for (h, w), c_in, c_out, n in itertools.product(SWEEP_PLANES, SWEEP_C, SWEEP_C, SWEEP_N):
            for v in var:
                c = (op, n, c_in, h, w, c_out) + v
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
    """integer operands as they lie in memory: x [n, c_in, h, w], w [c_out, c_in, 3, 3] (the buffer; layout says how it is read),
    bias [c_out], gy [n, c_out, h_out, w_out]"""
    op, n, c_in, h, w, c_out = case[:6]
    rng = np.random.default_rng([seed, 2, op, n, c_in, h, w, c_out])
    ho, wo = out_hw(h, w)
    x = rng.integers(-4, 5, (n, c_in, h, w), dtype=np.int8).astype(f32)
    wt = rng.integers(-4, 5, (c_out, c_in, 3, 3), dtype=np.int8).astype(f32)
    bias = rng.integers(-8, 9, c_out).astype(f32)
    gy = rng.integers(-4, 5, (n, c_out, ho, wo), dtype=np.int8).astype(f32)
    return x, wt, bias, gy


def initial(case, shape, seed=1):
    """the integer y0 an accumulating call starts from"""
    return np.random.default_rng([seed, 2] + [int(v) & 0xFFFF for v in case[:6]]).integers(-8, 9, shape).astype(f32)


def dilate(gy, h, w):
    """gy at [::2, ::2] of zeros [n, c_out, h, w]"""
    n, c_out = gy.shape[:2]
    g = np.zeros((n, c_out, h, w), gy.dtype)
    g[:, :, ::2, ::2] = gy
    return g


def forward(x, wt, bias, layout, relu):
    """[n, c_out, h_out, w_out] float32"""
    return np.ascontiguousarray(conv_ref.forward(x, wt, bias, 1, layout, relu)[:, :, ::2, ::2])


def input_grad(gy, wt, c_in, h, w, layout):
    """[n, c_in, h, w] float32"""
    return conv_ref.input_grad(dilate(gy, h, w), wt, c_in, layout)


def weight_grad(x, gy, layout):
    """[c_out, c_in, 3, 3] float32 as the gradient lies in memory under `layout`"""
    return conv_ref.weight_grad(x, dilate(gy, x.shape[2], x.shape[3]), 1, layout)


# ---------------------------------------------------------------------------------------------------------------- the GPU case table
def _c(op, n, c_in, h, w, c_out, layout=0, relu_bias=None, acc=0, w_off=0):
    return (op, n, c_in, h, w, c_out, layout, (3 if op == FWD else 0) if relu_bias is None else relu_bias, acc, w_off)


PLANES = ((1, 1), (2, 2), (5, 6), (6, 5), (7, 2), (33, 20))      # even and odd sides (the dropped tap of an even side), two row bands, the last ragged
NAMED_CASES = tuple(
    # ---- every plane, three images, a second channel pass of one channel past 8 and a channel tile of one channel past 16, both layouts
    [_c(op, 3, 9, h, w, 17, layout=lay) for op in range(3) for h, w in PLANES for lay in (0, 1)]
    # ---- and the other way round for the input gradient (c_in takes the channel tiles, c_out the passes)
    + [_c(BWD_INPUT, 3, 17, h, w, 9) for h, w in PLANES]
    # ---- channel counts around a pass (8) and a tile (16), one image
    + [_c(op, 1, ci, 5, 6, co) for op in range(3) for ci in (1, 3, 8, 9) for co in (1, 5, 16, 17)]
    # ---- one image past a whole image group (5 x 6 -> 3 x 3: groups of 14 images, of 10 in the weight gradient) and one image alone
    + [_c(op, n, 8, 5, 6, 16) for op in range(3) for n in (1, 15)]
    # ---- accumulate on both gradients, both layouts
    + [_c(op, 3, 9, h, w, 17, layout=lay, acc=1) for op in (BWD_INPUT, BWD_WEIGHT) for h, w in ((6, 5), (33, 20)) for lay in (0, 1)]
    # ---- the four bias x ReLU combinations
    + [_c(FWD, 3, 9, 6, 5, 17, relu_bias=rb) for rb in range(4)]
    # ---- a weight pointer and a gw pointer 4 bytes past a 16-byte boundary
    + [_c(FWD, 3, 8, 6, 5, 16, w_off=4), _c(BWD_INPUT, 3, 8, 6, 5, 16, w_off=4)] + [_c(BWD_WEIGHT, 3, 8, 6, 5, 16, acc=a, w_off=4) for a in (0, 1)]
    # ---- rows cut into column blocks (w_out = 150: two blocks of 75, in the weight gradient three of 50), the last column of an even width
    + [_c(op, 2, 3, 4, 300, 5) for op in range(3)] + [_c(op, 2, 3, 3, 299, 5, layout=1) for op in range(3)]
    # ---- the weight gradient's G: 16 pixel-block classes (slab_sum_kernel) and 15 (th_colsum)
    + [_c(BWD_WEIGHT, 16, 8, 33, 20, 16), _c(BWD_WEIGHT, 15, 8, 16, 20, 16)]
)

# the smallest shape of the sweep for every form the named cases above do not reach (regenerate: python -m tests.conv_s2_ref)
GENERATED_CASES = [
    (0, 1, 1, 3, 300, 17, 0, 3, 0, 0),   # s2_fwd: conv3x3_s2_fwd_kernel<CT=2> column blocks
    (0, 96, 1, 3, 255, 65, 0, 3, 0, 0),   # s2_fwd: conv3x3_s2_fwd_kernel<CT=4>
    (0, 96, 1, 3, 300, 64, 0, 3, 0, 0),   # s2_fwd: conv3x3_s2_fwd_kernel<CT=4> column blocks
    (1, 1, 1, 3, 300, 1, 0, 0, 1, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=1> accumulate=1 column blocks
    (1, 1, 17, 3, 300, 1, 0, 0, 0, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=2> accumulate=0 column blocks
    (1, 1, 17, 1, 1, 1, 0, 0, 1, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=2> accumulate=1
    (1, 1, 17, 3, 300, 1, 0, 0, 1, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=2> accumulate=1 column blocks
    (1, 96, 65, 3, 255, 1, 0, 0, 0, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=4> accumulate=0
    (1, 96, 64, 3, 300, 1, 0, 0, 0, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=4> accumulate=0 column blocks
    (1, 96, 65, 3, 255, 1, 0, 0, 1, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=4> accumulate=1
    (1, 96, 64, 3, 300, 1, 0, 0, 1, 0),   # s2_bwd_input: conv3x3_s2_bwd_input_kernel<CT=4> accumulate=1 column blocks
    (2, 9, 1, 3, 255, 16, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=1> slab_sum_kernel column blocks
    (2, 1, 1, 3, 255, 16, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=1> th_colsum column blocks
    (2, 1, 1, 3, 255, 16, 0, 0, 1, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=1> th_colsum_accum column blocks
    (2, 1536, 1, 1, 1, 32, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> slab_sum_kernel
    (2, 9, 1, 3, 255, 32, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> slab_sum_kernel column blocks
    (2, 1, 1, 1, 1, 32, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> th_colsum
    (2, 1, 1, 3, 255, 32, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> th_colsum column blocks
    (2, 1, 1, 1, 1, 32, 0, 0, 1, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> th_colsum_accum
    (2, 1, 1, 3, 255, 32, 0, 0, 1, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> th_colsum_accum column blocks
    (2, 1, 1, 3, 255, 17, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=2> th_colsum + wgrad_scatter_kernel column blocks
    (2, 1536, 1, 1, 1, 64, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> slab_sum_kernel
    (2, 9, 1, 3, 255, 64, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> slab_sum_kernel column blocks
    (2, 1, 1, 1, 1, 64, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum
    (2, 1, 1, 3, 255, 64, 0, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum column blocks
    (2, 1, 1, 1, 1, 64, 0, 0, 1, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum_accum
    (2, 1, 1, 3, 255, 64, 0, 0, 1, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum_accum column blocks
    (2, 1, 1, 1, 1, 64, 1, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum + wgrad_scatter_kernel
    (2, 1, 1, 3, 255, 64, 1, 0, 0, 0),   # s2_bwd_weight: conv3x3_s2_wgrad_kernel<CT=4> th_colsum + wgrad_scatter_kernel column blocks
]

CASES = list(dict.fromkeys(list(NAMED_CASES) + GENERATED_CASES))


def case_id(c):
    op, n, c_in, h, w, c_out, lay, rb, acc, off = c
    return (f"{OP_NAMES[op]}-{n}x{c_in}x{h}x{w}-{c_out}-l{lay}" + ("" if rb == (3 if op == FWD else 0) else f"-rb{rb}") + ("-acc" if acc else "") +
            ("-off" if off else ""))


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
