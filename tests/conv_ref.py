"""Shared by tests/test_conv_plan.py (no GPU) and tests/test_gpu_conv_forms.py: th_debug_conv3x3_plan as a dict, the sweep that finds every
reachable kernel form of the 3x3 convolution entry points (csrc/conv_pool.hip, conv_mfma.hip, conv_chain.hip), the GPU case table, and the
exact reference.

A CASE is (op, n, c_in, h, w, c_out, pad, layout, relu_bias, accumulate, w_off, img_mode): op 0 th_conv3x3_fwd, 1 _pool2_fwd, 2 _gap_fwd,
3 _bwd_input, 4 _bwd_weight; relu_bias = relu + 2 * (bias present); w_off: bytes of the weight pointer (op 4: of gw) off a 16-byte boundary;
img_mode: th_debug_set_conv_img.  A FORM is (op, family, the family's template parameters and path switches): what decides which kernel
instance runs and which of its paths -- see form_of.

Exactness.  x, w and gy are integers in [-4, 4], bias and the initial output (accumulate) integers in [-8, 8].  A forward output or an input
gradient is a sum of 9 max(c_in, c_out) products of magnitude <= 16 plus a bias / initial value: |sum| <= 16 * 9 * max(c_in, c_out) + 16
(150 channels: 21 616).  A weight gradient sums one product per output pixel: |sum| <= 16 * n * h_out * w_out + 8 (128 x 28 x 28 pixels:
1 605 640).  Every partial sum of either is an integer below 2^24, so float32 holds each exactly: every summation order, MFMA chain, slab
order and reduce ending gives the float32 bits of numpy's float64 result.  The one rounding is the global mean: an exact integer plane sum
divided by the pixel count in float32 (the kernels compute `sum / (float)pixels`, a correctly rounded division) -- restated as exactly that."""
import ctypes as C
import functools
import itertools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

f32 = np.float32
PLAN_FIELDS = ("family", "ct", "acc", "cit", "pool", "wh", "dma", "tpw", "wp", "cis", "px", "prep", "img_t", "rows_t", "bands", "grid_x", "grid_y",
               "grid_z", "tile_store", "gap", "lds", "lds_limit", "post", "lin", "G", "slabs", "reduce", "pq", "n_pb", "co_ld", "refused", "h_out",
               "w_out")
REFUSED, CONV1, TILE, ROWS, MFMA, IMG, CHAIN, WGRAD_MFMA, WGRAD_IMG, WGRAD_CONV1, WGRAD_VEC = range(11)
FAMILY_NAMES = ("refused", "conv1_kernel", "conv3x3_kernel", "conv3x3_rows_kernel", "conv3x3_mfma_kernel", "conv3x3_img_kernel",
                "conv_layer_chain_kernel", "conv3x3_wgrad_mfma_kernel", "conv_wgrad_img_kernel", "conv1_wgrad_kernel", "conv3x3_bwd_weight_kernel")
R_NONE, R_SLAB_SUM, R_COLSUM, R_COLSUM_ACCUM, R_SCATTER = range(5)
REDUCE_NAMES = ("-", "slab_sum_kernel", "th_colsum", "th_colsum_accum", "th_colsum + wgrad_scatter_kernel")
REFUSAL_NAMES = ("-", "plane over the LDS tile", "no gap plan", "no pool plan", "pad", "weight-gradient limits")
OP_NAMES = ("fwd", "pool2", "gap", "bwd_input", "bwd_weight")
FWD, POOL2, GAP, BWD_INPUT, BWD_WEIGHT = range(5)


def _lib():
    from taper_amd._lib import hip
    return hip


def plan(op, n, c_in, h, w, c_out, pad=1, layout=0, relu_bias=3, acc=0, w_off=0, img_mode=-1):
    """th_debug_conv3x3_plan as a dict (pure host code: no context, no device)"""
    out = (C.c_int * len(PLAN_FIELDS))()
    assert _lib().th_debug_conv3x3_plan(op, n, c_in, h, w, c_out, pad, layout, relu_bias, acc, w_off, img_mode, C.cast(out, C.c_void_p)) == 0, \
        _lib().th_last_error()
    return dict(zip(PLAN_FIELDS, out))


def form_of(*case):
    return form_from(case, plan(*case))


def form_from(case, p):
    op, n, c_in, h, w, c_out = case[:6]
    fam = p["family"]
    if fam == REFUSED:
        return (op, fam, p["refused"])
    if fam == CONV1:
        return (op, fam, p["pool"])
    if fam == TILE:
        return (op, fam, p["acc"])
    if fam == ROWS:
        return (op, fam, p["px"], p["acc"])
    if fam == MFMA:
        return (op, fam, p["ct"], p["acc"], p["cit"], p["pool"], p["wh"], p["dma"], p["prep"])
    if fam == IMG:
        return (op, fam, p["ct"], p["tpw"], p["pool"], p["wp"], p["gap"], p["tile_store"], p["prep"])
    if fam == CHAIN:      # the instance is its geometry: (S, C_IN, C_OUT) as the kernel sees them (an input gradient swaps the channels)
        return (op, fam, h) + ((c_out, c_in) if op == BWD_INPUT else (c_in, c_out)) + (p["post"], p["lin"])
    if fam == WGRAD_MFMA:
        return (op, fam, p["ct"], p["pq"], p["reduce"])
    if fam == WGRAD_IMG:
        return (op, fam, h, c_in, c_out, p["reduce"])
    if fam == WGRAD_CONV1:
        return (op, fam, p["reduce"])
    return (op, fam, int(p["slabs"] > 0), p["reduce"], p["acc"])


def form_name(f):
    op, fam = f[:2]
    s = f"{OP_NAMES[op]}: {FAMILY_NAMES[fam]}"
    if fam == REFUSED:
        return s + f" ({REFUSAL_NAMES[f[2]]})"
    if fam == CONV1:
        return f"{OP_NAMES[op]}: " + ("conv1_pool2_kernel" if f[2] else "conv1_kernel")
    if fam == TILE:
        return s + f"<ACC={f[2]}>"
    if fam == ROWS:
        return s + f"<PX={f[2]}, ACC={f[3]}>"
    if fam == MFMA:
        return s + f"<CT={f[2]}, ACC={f[3]}, CIT={f[4]}, POOL={f[5]}, WH={f[6]}, DMA={f[7]}>" + (" prepped weights" if f[8] else " weights in place")
    if fam == IMG:
        return (s + f"<CT={f[2]}, TPW={f[3]}, POOL={f[4]}, WP={f[5]}>" + (" gap" if f[6] else "") + (" tile_store" if f[7] else "") +
                (" prepped weights" if f[8] else " weights in place"))
    if fam == CHAIN:
        return s + f"<S={f[2]}, C_IN={f[3]}, C_OUT={f[4]}, POST={f[5]}, LIN={f[6]}>"
    if fam == WGRAD_MFMA:
        return s + f"<CT={f[2]}, PQ={f[3]}> {REDUCE_NAMES[f[4]]}"
    if fam == WGRAD_IMG:
        return s + f"<S={f[2]}, C_IN={f[3]}, C_OUT={f[4]}> {REDUCE_NAMES[f[5]]}"
    if fam == WGRAD_CONV1:
        return s + f" {REDUCE_NAMES[f[2]]}"
    return s + (f" image slabs, {REDUCE_NAMES[f[3]]}" if f[2] else " into gw") + f", accumulate={f[4]}"


# ---------------------------------------------------------------------------------------------------------------- the sweep
SWEEP_C_IN = (1, 2, 7, 8, 9, 13, 16, 24, 32, 40, 64, 128)
SWEEP_C_OUT = (1, 4, 7, 16, 17, 32, 33, 48, 64, 70, 128, 150)
SWEEP_N = (1, 2, 3, 9, 31, 32, 127, 128, 129, 131, 257)
# (h_out, w_out): 1 x 1 and 3 x 3 through 7, 14, 28, 30; odd and rectangular; the widest matrix-core plane (w_out = 126) and 127 (the vector
# ALUs take it); the pool limit (w_out = 64 / 66); one input channel on a plane over 48 KB (110 x 110, and 186 x 64 which the pool accepts); a
# plane the vector-ALU tile cannot hold (72 x 72 with 8-channel passes: 175 KB)
SWEEP_PLANES = ((1, 1), (3, 3), (7, 7), (14, 14), (28, 28), (30, 30), (5, 9), (9, 6), (3, 40), (4, 126), (4, 127), (6, 64), (6, 66), (72, 72),
                (110, 110), (186, 64))


def _variants(op):
    """(pad, layout, relu_bias, accumulate, w_off, img_mode) an op's dispatch can tell apart"""
    if op == FWD:      # a misaligned pointer matters to the in-place path (layout 0) alone; ReLU / bias to the chain (default mode) alone
        return [(pad, lay, rb, 0, off, im) for pad in (0, 1) for lay, off in ((0, 0), (0, 4), (1, 0))
                for im, rb in ((-1, 3), (-1, 0), (0, 3), (1, 3))]
    if op in (POOL2, GAP):
        return [(pad, 0, 3, 0, off, im) for pad in (0, 1) for off, im in ((0, -1), (0, 0), (0, 1), (4, -1))]
    if op == BWD_INPUT:
        return [(1, lay, 0, acc, 0, im) for lay in (0, 1) for acc in (0, 1) for im in (-1, 0, 1)]
    return [(pad, lay, 0, acc, off, -1) for pad in (0, 1) for lay in (0, 1) for acc in (0, 1) for off in (0, 4)]


def _size(c):
    return c[1] * c[2] * c[3] * c[4] * c[5]


def violations(case, p):
    """what any launch needs of its plan, and what the entry points promise of it: [] or the broken invariants of plan p of `case`"""
    op, n, c_in, h, w, c_out, pad, lay, rb, acc, off, im = case
    fam, bad = p["family"], []
    if op == POOL2 and (fam != REFUSED) != bool(_lib().th_conv3x3_pool2_supported(c_in, h, w, c_out, pad) and off == 0):
        bad.append("th_conv3x3_pool2_supported disagrees with the plan")
    if op == GAP and (fam != REFUSED) != bool(_lib().th_conv3x3_gap_supported(n, c_in, h, w, c_out, pad) and off == 0):
        bad.append("th_conv3x3_gap_supported disagrees with the plan")
    if fam == REFUSED:
        return bad + ([] if p["refused"] else ["refused without a reason"])
    if p["refused"]:
        bad.append("a reason to refuse on a plan that launches")
    if p["img_t"] < 1 or min(p["grid_x"], p["grid_y"], p["grid_z"]) < 1:
        bad.append("img_t or a grid dimension below 1")
    if fam in (MFMA, WGRAD_MFMA) and not (1 <= p["rows_t"] and p["rows_t"] * p["w_out"] <= 128 and p["bands"] == -(-p["h_out"] // p["rows_t"])):
        bad.append("rows_t * w_out over 128 pixels, or bands do not tile h_out")
    if not 0 <= p["lds"] <= p["lds_limit"] <= 160 << 10:
        bad.append("LDS over the limit the launch requests")
    if fam == WGRAD_MFMA and not 1 <= p["G"] <= min(p["n_pb"], 512):
        bad.append("G over min(n_pb, 512)")
    if op == BWD_WEIGHT and (p["slabs"] > 0) != (p["reduce"] != R_NONE):
        bad.append("slabs without a reduce ending, or an ending without slabs")
    if op == BWD_WEIGHT and p["reduce"] == R_SLAB_SUM and not (lay == 0 and off == 0 and p["slabs"] >= 16 and 9 * c_in * c_out % 4 == 0):
        bad.append("slab_sum_kernel needs 16 slabs, whole quads and an aligned gw in the taper layout")
    if op <= GAP and fam in (MFMA, IMG, CHAIN) and not p["prep"] and not (lay == 0 and c_out % 4 == 0 and off == 0):
        bad.append("weights read in place without c_out % 4 == 0 and an aligned pointer")
    if bool(p["gap"]) != (op == GAP) or bool(p["pool"]) != (op in (POOL2, GAP)):
        bad.append("a gap / pool form outside its op")
    if fam == CHAIN and not (n >= 128 and im == -1 and pad == 1 and h == w and not acc):
        bad.append("a one-stage chain below 128 images, off the default mode, or accumulating")
    return bad


@functools.lru_cache(maxsize=None)
def sweep():
    """one pass over the sweep -> ({form: the smallest case (by n c_in h w c_out) that reaches it}, [(case, broken invariant)])"""
    found, bad = {}, []
    for op in range(5):
        var = _variants(op)
        for (ho, wo), c_in, c_out, n in itertools.product(SWEEP_PLANES, SWEEP_C_IN, SWEEP_C_OUT, SWEEP_N):
            for v in var:
                pad = v[0]
                c = (op, n, c_in, ho + 2 - 2 * pad, wo + 2 - 2 * pad, c_out) + v
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
    op, n, c_in, h, w, c_out, pad = case[:7]
    rng = np.random.default_rng([seed, op, n, c_in, h, w, c_out, pad])
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    x = rng.integers(-4, 5, (n, c_in, h, w), dtype=np.int8).astype(f32)
    wt = rng.integers(-4, 5, (c_out, c_in, 3, 3), dtype=np.int8).astype(f32)
    bias = rng.integers(-8, 9, c_out).astype(f32)
    gy = rng.integers(-4, 5, (n, c_out, ho, wo), dtype=np.int8).astype(f32)
    return x, wt, bias, gy


def initial(case, shape, seed=1):
    """the integer y0 an accumulating call starts from"""
    return np.random.default_rng([seed] + [int(v) & 0xFFFF for v in case[:7]]).integers(-8, 9, shape).astype(f32)


def patches(x, pad):
    """[n * h_out * w_out, c_in * 9] float64: the 3x3 windows of the zero-padded planes, k = (ci, kh, kw)"""
    n, c, h, w = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    win = sliding_window_view(xp, (3, 3), axis=(2, 3))                  # [n, c, ho, wo, 3, 3]
    ho, wo = win.shape[2:4]
    return np.ascontiguousarray(win.transpose(0, 2, 3, 1, 4, 5)).reshape(n * ho * wo, c * 9), ho, wo


def weight_matrix(wt, layout):
    """[9 c_in, c_out] float64.  layout 0: the reference's reinterpretation of the buffer as it lies; 1: the standard filter [co][ci][kh][kw]"""
    c_out = wt.shape[0]
    k = wt.size // c_out
    flat = wt.astype(np.float64).reshape(-1)
    return flat.reshape(k, c_out) if layout == 0 else flat.reshape(c_out, k).T


def _chunks(n, per_image):
    """image ranges whose patch matrix stays below 16 M float64 values"""
    step = max(1, (1 << 24) // max(1, per_image))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def _conv(x, wm, pad):
    """x [n, c, h, w] convolved with the matrix wm [9 c, c_out] -> [n, c_out, h_out, w_out] float64"""
    n, c, h, w = x.shape
    out = []
    for lo, hi in _chunks(n, c * 9 * (h + 2 * pad - 2) * (w + 2 * pad - 2)):
        p, ho, wo = patches(x[lo:hi], pad)
        out.append((p @ wm).reshape(hi - lo, ho, wo, wm.shape[1]).transpose(0, 3, 1, 2))
    return np.concatenate(out)


def forward(x, wt, bias, pad, layout, relu):
    """[n, c_out, h_out, w_out] float32"""
    y = _conv(x, weight_matrix(wt, layout), pad)
    if bias is not None:
        y = y + bias.astype(np.float64)[None, :, None, None]
    if relu:
        y = np.where(y > 0, y, 0.0)
    return np.ascontiguousarray(y).astype(f32)


def pool2(y):
    """2 x 2 / stride 2 maximum (whole windows)"""
    n, c, h, w = y.shape
    return np.ascontiguousarray(y.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5)))


def gap(y):
    """(plane means, counts of outputs > 0) [n, c_out]: the exact plane sum divided by the pixel count in float32, as the kernels do"""
    n, c, h, w = y.shape
    s = y.astype(np.float64).sum(axis=(2, 3))
    assert np.abs(s).max() < 2 ** 24
    return s.astype(f32) / f32(h * w), (y > 0).sum(axis=(2, 3)).astype(f32)


def input_grad(gy, wt, c_in, layout):
    """[n, c_in, h, w] float32 of a pad-1 convolution: gy convolved with the mirrored filter, channels swapped"""
    c_out = gy.shape[1]
    std = weight_matrix(wt, layout).T.reshape(c_out, c_in, 3, 3)          # [co][ci][kh][kw]
    mir = np.ascontiguousarray(std[:, :, ::-1, ::-1].transpose(0, 2, 3, 1)).reshape(c_out * 9, c_in)      # [(co, kh, kw)][ci]
    return np.ascontiguousarray(_conv(gy, mir, 1)).astype(f32)


def weight_grad(x, gy, pad, layout):
    """[c_out, c_in, 3, 3] float32 as the gradient lies in memory under `layout`"""
    n, c_in, h, w = x.shape
    c_out = gy.shape[1]
    g = np.zeros((9 * c_in, c_out))
    for lo, hi in _chunks(n, c_in * 9 * (h + 2 * pad - 2) * (w + 2 * pad - 2)):
        p, ho, wo = patches(x[lo:hi], pad)
        g += p.T @ gy[lo:hi].astype(np.float64).transpose(0, 2, 3, 1).reshape((hi - lo) * ho * wo, c_out)      # [9 c_in, c_out]
    return np.ascontiguousarray(g if layout == 0 else g.T).astype(f32).reshape(c_out, c_in, 3, 3)


# ---------------------------------------------------------------------------------------------------------------- the GPU case table
def _c(op, n, c_in, h, w, c_out, pad=1, layout=0, relu_bias=None, acc=0, w_off=0, img_mode=-1):
    return (op, n, c_in, h, w, c_out, pad, layout, (3 if op <= GAP else 0) if relu_bias is None else relu_bias, acc, w_off, img_mode)


NAMED_CASES = tuple(
    # ---- ragged geometry on the 128-pixel matrix-core kernel (img_mode 0 keeps the image-resident kernel off): 14 rows in bands of 9 (the
    #      last band has 5); 11 images in groups of 9; c_in = 9 / 13: a second pass of one / five channels past c_in, no DMA
    [_c(FWD, 2, 8, 14, 14, 16, img_mode=0), _c(FWD, 11, 9, 7, 7, 17), _c(FWD, 3, 13, 9, 11, 33, pad=0), _c(FWD, 3, 13, 9, 11, 33, layout=1)]
    # ---- c_out one past a multiple of the channel block: forward (prepped weights, the last channel tile holds one channel), input gradient
    #      (c_in takes that role), weight gradient (co_ld > c_out: the scatter ending)
    + [_c(FWD, 3, 8, 9, 11, co) for co in (17, 33, 65, 129)] + [_c(BWD_INPUT, 3, ci, 9, 11, 8) for ci in (17, 33, 65, 129)]
    + [_c(BWD_WEIGHT, 12, 16, 14, 14, co) for co in (17, 33, 65, 129)]
    # ---- c_in % 16 != 0 in the weight-gradient slab (9: one slab of nine channels; 24: a second slab of eight), both layouts
    + [_c(BWD_WEIGHT, 50, 9, 7, 7, 16, layout=lay) for lay in (0, 1)] + [_c(BWD_WEIGHT, 12, 24, 14, 14, 24, layout=lay) for lay in (0, 1)]
    # ---- limits: the widest matrix-core plane (w_out = 126) and 127, which the vector ALUs take; the pool at w_out = 64; c_in = 1 in layout 1
    #      (CIT = 1 on the matrix cores); c_in = 1 on a plane over 48 KB (112 x 112 floats with the halo: 50 176 B; 188 x 66 for the pool, whose rows hold <= 64 outputs)
    + [_c(FWD, 1, 8, 4, 126, 4), _c(FWD, 1, 8, 4, 127, 4), _c(FWD, 1, 8, 6, 128, 8, pad=0), _c(POOL2, 2, 8, 6, 64, 4), _c(POOL2, 2, 8, 6, 66, 4),
       _c(FWD, 3, 1, 9, 7, 20, layout=1), _c(POOL2, 3, 1, 28, 28, 32), _c(FWD, 1, 1, 110, 110, 4), _c(FWD, 1, 1, 110, 110, 4, layout=1),
       _c(POOL2, 1, 1, 186, 64, 4)]
    # ---- switch thresholds of the 128-pixel kernel (c_in = 9: never the image-resident kernel): 188 x 2 = 376 < 384 workgroup slots -> CT 2,
    #      192 x 2 = 384 -> CT 4; 764 workgroups -> WH 2, 768 -> WH 1
    + [_c(FWD, 423, 9, 7, 7, 128), _c(FWD, 424, 9, 7, 7, 128), _c(FWD, 1719, 9, 7, 7, 32), _c(FWD, 1720, 9, 7, 7, 32)]
    # ---- tile_store of the image-resident kernel just below and at 2^19 outputs (167 / 168 x 16 x 196 = 523 712 / 526 848)
    + [_c(FWD, 167, 8, 14, 14, 16), _c(FWD, 168, 8, 14, 14, 16)]
    # ---- batch edges of the one-stage chains and the image-resident weight gradient: 127 images take the layer-by-layer kernels, 128 and 129
    #      the compiled chain / image form (an image per workgroup)
    + [_c(op, n, ci, s, s, co) for n in (127, 128, 129) for op, ci, s, co in (
        (FWD, 32, 28, 32), (FWD, 32, 14, 64), (FWD, 64, 14, 64), (FWD, 64, 7, 128), (POOL2, 32, 28, 32), (POOL2, 32, 14, 64), (POOL2, 64, 14, 64),
        (GAP, 64, 7, 128), (BWD_INPUT, 32, 14, 64), (BWD_INPUT, 64, 7, 128), (BWD_INPUT, 32, 28, 32), (BWD_INPUT, 64, 14, 64),
        (BWD_WEIGHT, 32, 14, 64), (BWD_WEIGHT, 64, 14, 64), (BWD_WEIGHT, 32, 28, 32))]
    # ---- the chain's conditions from the other side: no ReLU with a bias, accumulate -> the layer-by-layer kernels at batch 128; no ReLU and
    #      no bias: the LIN chain from the forward entry point; layout 1: the chain over prepped weights (128 channels need no padding)
    + [_c(FWD, 128, 64, 7, 7, 128, relu_bias=2), _c(FWD, 128, 64, 7, 7, 128, relu_bias=0), _c(BWD_INPUT, 128, 64, 7, 7, 128, acc=1),
       _c(FWD, 128, 64, 7, 7, 128, layout=1)]
    # ---- weight gradient: PQ = 2 (a patch chunk of 14 images x 25 floats > 256); G clamped by the pixel blocks (21) and by 512 (525 blocks)
    + [_c(BWD_WEIGHT, 257, 8, 3, 3, 16), _c(BWD_WEIGHT, 11, 8, 14, 14, 16), _c(BWD_WEIGHT, 300, 8, 14, 14, 16)]
    # ---- wgrad_reduce: G = 15 (th_colsum, odd cols = 27 x 23) / 16 (slab_sum_kernel) image slabs of conv3x3_bwd_weight_kernel; G = 16 pixel-block
    #      classes of the matrix-core kernel; a gw 4 bytes off the boundary (th_colsum / th_colsum_accum instead); layout 1 (the scatter ending)
    + [_c(BWD_WEIGHT, 15, 3, 24, 24, 23, acc=a) for a in (0, 1)] + [_c(BWD_WEIGHT, 16, 2, 24, 24, 32, acc=a, w_off=o) for a in (0, 1) for o in (0, 4)]
    + [_c(BWD_WEIGHT, 8, 8, 16, 16, 16, acc=a, w_off=o) for a in (0, 1) for o in (0, 4)] + [_c(BWD_WEIGHT, 8, 8, 16, 16, 16, layout=1, acc=1)]
    + [_c(BWD_WEIGHT, 40, 1, 28, 28, 32, layout=lay, acc=a) for lay in (0, 1) for a in (0, 1)]
    # ---- both forced modes of th_debug_set_conv_img on one shape per op it reaches (3 x 32 x 14 x 14 -> 64: the default takes the 128-pixel kernel)
    + [_c(op, 3, 32, 14, 14, 64, img_mode=im) for op in (FWD, POOL2, BWD_INPUT) for im in (0, 1)]
    # ---- shapes the vector-ALU path must refuse: (h + 2)(w + 2) x 32 B = 175 KB over the 160 KB tile (forward, and the input gradient of c_out = 3)
    + [_c(FWD, 2, 3, 72, 72, 4), _c(BWD_INPUT, 2, 4, 72, 72, 3)]
    # ---- vector-ALU kernels on more than one workgroup and channel block: PX 4 / 2 / 1 rows, the 2 x 4 tiles, accumulate
    + [_c(FWD, 5, 3, 8, 8, 20, pad=0), _c(FWD, 2, 5, 9, 6, 7), _c(FWD, 7, 7, 7, 7, 17), _c(FWD, 3, 4, 8, 16, 20), _c(BWD_INPUT, 3, 20, 8, 16, 4, acc=1),
       _c(BWD_INPUT, 7, 17, 7, 7, 7, acc=1)]
)

# the smallest shape of the sweep for every form the named cases above do not reach (regenerate: python -m tests.conv_ref)
GENERATED_CASES = [
    (1, 9, 1, 186, 64, 32, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=1, WH=1, DMA=0> weights in place
    (1, 1, 1, 186, 64, 32, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=1, WH=2, DMA=0> weights in place
    (1, 9, 1, 186, 64, 64, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=1, WH=1, DMA=0> weights in place
    (1, 3, 1, 186, 64, 128, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=1, WH=2, DMA=0> weights in place
    (0, 1, 1, 1, 1, 1, 1, 0, 3, 0, 0, -1),   # fwd: conv1_kernel
    (0, 1, 2, 3, 40, 1, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_rows_kernel<PX=4, ACC=0>
    (0, 1, 8, 1, 1, 1, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=1, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (0, 9, 1, 110, 110, 32, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> weights in place
    (0, 128, 1, 6, 66, 17, 1, 1, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (0, 1, 1, 110, 110, 32, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=0, WH=2, DMA=0> weights in place
    (0, 128, 9, 6, 66, 17, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (0, 9, 1, 110, 110, 64, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> weights in place
    (0, 128, 1, 6, 66, 64, 1, 1, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (0, 2, 1, 110, 110, 128, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=2, DMA=0> weights in place
    (0, 32, 1, 6, 66, 70, 1, 1, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=2, DMA=0> prepped weights
    (0, 128, 9, 6, 66, 64, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> weights in place
    (0, 128, 9, 6, 66, 64, 1, 0, 3, 0, 4, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (0, 32, 8, 6, 66, 128, 1, 0, 3, 0, 0, 0),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=1> weights in place
    (0, 32, 8, 6, 66, 70, 1, 0, 3, 0, 0, 0),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=1> prepped weights
    (0, 32, 9, 6, 66, 70, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=2, DMA=0> prepped weights
    (0, 1, 8, 1, 1, 1, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=4, POOL=0, WP=0> prepped weights
    (0, 32, 8, 4, 126, 33, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=4, POOL=0, WP=0> tile_store prepped weights
    (0, 1, 8, 28, 28, 4, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=0> weights in place
    (0, 1, 8, 28, 28, 1, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=0> prepped weights
    (0, 127, 8, 28, 28, 7, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=0> tile_store prepped weights
    (0, 257, 8, 14, 14, 48, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=16> tile_store weights in place
    (0, 257, 8, 14, 14, 33, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=16> tile_store prepped weights
    (0, 1, 8, 30, 30, 4, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> weights in place
    (0, 1, 8, 30, 30, 1, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> prepped weights
    (0, 31, 8, 30, 30, 32, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> tile_store weights in place
    (0, 9, 8, 30, 30, 70, 1, 0, 3, 0, 0, 1),   # fwd: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> tile_store prepped weights
    (0, 127, 8, 1, 1, 48, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> weights in place
    (0, 127, 8, 1, 1, 33, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> prepped weights
    (0, 127, 8, 3, 40, 48, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> tile_store weights in place
    (0, 127, 8, 3, 40, 48, 1, 0, 3, 0, 4, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> tile_store prepped weights
    (0, 257, 8, 3, 40, 64, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=7, POOL=0, WP=0> tile_store weights in place
    (0, 127, 8, 6, 64, 33, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=7, POOL=0, WP=0> tile_store prepped weights
    (0, 127, 8, 28, 28, 48, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=13, POOL=0, WP=30> tile_store weights in place
    (0, 127, 8, 28, 28, 33, 1, 0, 3, 0, 0, -1),   # fwd: conv3x3_img_kernel<CT=2, TPW=13, POOL=0, WP=30> tile_store prepped weights
    (0, 128, 128, 7, 7, 64, 1, 0, 0, 0, 0, -1),   # fwd: conv_layer_chain_kernel<S=7, C_IN=128, C_OUT=64, POST=0, LIN=1>
    (0, 128, 64, 14, 14, 32, 1, 0, 0, 0, 0, -1),   # fwd: conv_layer_chain_kernel<S=14, C_IN=64, C_OUT=32, POST=0, LIN=1>
    (0, 128, 64, 14, 14, 64, 1, 0, 0, 0, 0, -1),   # fwd: conv_layer_chain_kernel<S=14, C_IN=64, C_OUT=64, POST=0, LIN=1>
    (0, 128, 32, 28, 28, 32, 1, 0, 0, 0, 0, -1),   # fwd: conv_layer_chain_kernel<S=28, C_IN=32, C_OUT=32, POST=0, LIN=1>
    (1, 128, 9, 6, 64, 48, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=8, POOL=1, WH=1, DMA=0> weights in place
    (1, 1, 9, 14, 14, 32, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=8, POOL=1, WH=2, DMA=0> weights in place
    (1, 128, 9, 6, 64, 128, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=1, WH=1, DMA=0> weights in place
    (1, 31, 8, 28, 28, 128, 1, 0, 3, 0, 0, 0),   # pool2: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=1, WH=1, DMA=1> weights in place
    (1, 31, 9, 28, 28, 128, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=1, WH=2, DMA=0> weights in place
    (1, 257, 8, 14, 14, 48, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_img_kernel<CT=1, TPW=7, POOL=1, WP=16> weights in place
    (1, 1, 8, 30, 30, 4, 1, 0, 3, 0, 0, 1),   # pool2: conv3x3_img_kernel<CT=1, TPW=13, POOL=1, WP=0> weights in place
    (1, 127, 8, 14, 14, 48, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_img_kernel<CT=2, TPW=4, POOL=1, WP=0> weights in place
    (1, 127, 8, 6, 64, 48, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_img_kernel<CT=2, TPW=7, POOL=1, WP=0> weights in place
    (1, 127, 8, 28, 28, 48, 1, 0, 3, 0, 0, -1),   # pool2: conv3x3_img_kernel<CT=2, TPW=13, POOL=1, WP=30> weights in place
    (2, 1, 1, 1, 1, 1, 1, 0, 3, 0, 0, -1),   # gap: refused (no gap plan)
    (2, 1, 8, 28, 28, 4, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=1, TPW=7, POOL=1, WP=0> gap weights in place
    (2, 257, 8, 14, 14, 48, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=1, TPW=7, POOL=1, WP=16> gap weights in place
    (2, 1, 8, 30, 30, 4, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=1, TPW=13, POOL=1, WP=0> gap weights in place
    (2, 127, 8, 1, 1, 48, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=2, TPW=4, POOL=1, WP=0> gap weights in place
    (2, 257, 8, 3, 40, 64, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=2, TPW=7, POOL=1, WP=0> gap weights in place
    (2, 127, 8, 28, 28, 48, 1, 0, 3, 0, 0, -1),   # gap: conv3x3_img_kernel<CT=2, TPW=13, POOL=1, WP=30> gap weights in place
    (3, 1, 1, 6, 64, 4, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_kernel<ACC=0>
    (3, 1, 1, 1, 1, 4, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_rows_kernel<PX=1, ACC=0>
    (3, 1, 1, 9, 6, 4, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_rows_kernel<PX=2, ACC=0>
    (3, 1, 1, 9, 6, 4, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_rows_kernel<PX=2, ACC=1>
    (3, 1, 1, 3, 40, 4, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_rows_kernel<PX=4, ACC=0>
    (3, 1, 1, 3, 40, 4, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_rows_kernel<PX=4, ACC=1>
    (3, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=1, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 1, 1, 1, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=1, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=1, ACC=1, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 1, 1, 1, 16, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=1, ACC=1, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 128, 24, 6, 66, 1, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 24, 1, 1, 1, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=1, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 24, 6, 66, 17, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 24, 1, 1, 17, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=0, CIT=8, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 24, 6, 66, 1, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=1, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 1, 24, 1, 1, 1, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=1, CIT=1, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 24, 6, 66, 16, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=2, ACC=1, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 128, 64, 6, 66, 1, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 32, 128, 6, 66, 1, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=1, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 64, 6, 66, 17, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 32, 128, 6, 66, 16, 1, 0, 0, 0, 0, 0),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=1, DMA=1> prepped weights
    (3, 32, 128, 6, 66, 17, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=0, CIT=8, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 64, 6, 66, 1, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=1, CIT=1, POOL=0, WH=1, DMA=0> prepped weights
    (3, 32, 128, 6, 66, 1, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=1, CIT=1, POOL=0, WH=2, DMA=0> prepped weights
    (3, 128, 64, 6, 66, 16, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=1, CIT=8, POOL=0, WH=1, DMA=0> prepped weights
    (3, 32, 128, 6, 66, 16, 1, 0, 0, 1, 0, -1),   # bwd_input: conv3x3_mfma_kernel<CT=4, ACC=1, CIT=8, POOL=0, WH=2, DMA=0> prepped weights
    (3, 1, 1, 28, 28, 16, 1, 0, 0, 0, 0, 1),   # bwd_input: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=0> prepped weights
    (3, 257, 40, 14, 14, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_img_kernel<CT=1, TPW=7, POOL=0, WP=16> tile_store prepped weights
    (3, 1, 1, 30, 30, 16, 1, 0, 0, 0, 0, 1),   # bwd_input: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> prepped weights
    (3, 31, 24, 30, 30, 16, 1, 0, 0, 0, 0, 1),   # bwd_input: conv3x3_img_kernel<CT=1, TPW=13, POOL=0, WP=0> tile_store prepped weights
    (3, 127, 40, 1, 1, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> prepped weights
    (3, 127, 40, 3, 40, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_img_kernel<CT=2, TPW=4, POOL=0, WP=0> tile_store prepped weights
    (3, 127, 40, 6, 64, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_img_kernel<CT=2, TPW=7, POOL=0, WP=0> tile_store prepped weights
    (3, 127, 40, 28, 28, 16, 1, 0, 0, 0, 0, -1),   # bwd_input: conv3x3_img_kernel<CT=2, TPW=13, POOL=0, WP=30> tile_store prepped weights
    (4, 257, 8, 3, 3, 16, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=1, PQ=2> th_colsum
    (4, 257, 8, 3, 3, 16, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=1, PQ=2> th_colsum_accum
    (4, 3, 8, 28, 28, 32, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=1> th_colsum
    (4, 3, 8, 28, 28, 32, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=1> th_colsum_accum
    (4, 257, 8, 3, 3, 32, 1, 0, 0, 0, 0, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=2> slab_sum_kernel
    (4, 257, 8, 3, 3, 32, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=2> th_colsum
    (4, 257, 8, 3, 3, 32, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=2> th_colsum_accum
    (4, 257, 8, 3, 3, 17, 1, 0, 0, 0, 0, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=2, PQ=2> th_colsum + wgrad_scatter_kernel
    (4, 3, 8, 28, 28, 64, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=1> th_colsum
    (4, 3, 8, 28, 28, 64, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=1> th_colsum_accum
    (4, 257, 8, 3, 3, 64, 1, 0, 0, 0, 0, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=2> slab_sum_kernel
    (4, 257, 8, 3, 3, 64, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=2> th_colsum
    (4, 257, 8, 3, 3, 64, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=2> th_colsum_accum
    (4, 257, 8, 3, 3, 64, 1, 1, 0, 0, 0, -1),   # bwd_weight: conv3x3_wgrad_mfma_kernel<CT=4, PQ=2> th_colsum + wgrad_scatter_kernel
    (4, 128, 32, 14, 14, 64, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=32, C_OUT=64> th_colsum
    (4, 128, 32, 14, 14, 64, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=32, C_OUT=64> th_colsum_accum
    (4, 128, 32, 14, 14, 64, 1, 1, 0, 0, 0, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=32, C_OUT=64> th_colsum + wgrad_scatter_kernel
    (4, 128, 64, 14, 14, 64, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=64, C_OUT=64> th_colsum
    (4, 128, 64, 14, 14, 64, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=64, C_OUT=64> th_colsum_accum
    (4, 128, 64, 14, 14, 64, 1, 1, 0, 0, 0, -1),   # bwd_weight: conv_wgrad_img_kernel<S=14, C_IN=64, C_OUT=64> th_colsum + wgrad_scatter_kernel
    (4, 128, 32, 28, 28, 32, 1, 0, 0, 0, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=28, C_IN=32, C_OUT=32> th_colsum
    (4, 128, 32, 28, 28, 32, 1, 0, 0, 1, 4, -1),   # bwd_weight: conv_wgrad_img_kernel<S=28, C_IN=32, C_OUT=32> th_colsum_accum
    (4, 128, 32, 28, 28, 32, 1, 1, 0, 0, 0, -1),   # bwd_weight: conv_wgrad_img_kernel<S=28, C_IN=32, C_OUT=32> th_colsum + wgrad_scatter_kernel
    (4, 32, 1, 1, 1, 1, 1, 0, 0, 0, 0, -1),   # bwd_weight: conv1_wgrad_kernel th_colsum
    (4, 32, 1, 1, 1, 1, 1, 0, 0, 1, 0, -1),   # bwd_weight: conv1_wgrad_kernel th_colsum_accum
    (4, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, -1),   # bwd_weight: conv3x3_bwd_weight_kernel into gw, accumulate=0
    (4, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, -1),   # bwd_weight: conv3x3_bwd_weight_kernel into gw, accumulate=1
    (4, 2, 1, 72, 72, 1, 1, 1, 0, 0, 0, -1),   # bwd_weight: conv3x3_bwd_weight_kernel image slabs, th_colsum + wgrad_scatter_kernel, accumulate=0
    (4, 2, 1, 72, 72, 1, 1, 1, 0, 1, 0, -1),   # bwd_weight: conv3x3_bwd_weight_kernel image slabs, th_colsum + wgrad_scatter_kernel, accumulate=1
]

CASES = list(dict.fromkeys(list(NAMED_CASES) + GENERATED_CASES))


def case_id(c):
    op, n, c_in, h, w, c_out, pad, lay, rb, acc, off, im = c
    return (f"{OP_NAMES[op]}-{n}x{c_in}x{h}x{w}-{c_out}-p{pad}l{lay}" + ("" if rb == (3 if op <= GAP else 0) else f"-rb{rb}") +
            ("-acc" if acc else "") + ("-off" if off else "") + ("" if im == -1 else f"-img{im}"))


def cases_by_form():
    out = {}
    for c in CASES:
        out.setdefault(form_of(*c), []).append(c)
    return out


_FORM_PARAMS = {REFUSED: ("reason",), CONV1: ("POOL",), TILE: ("ACC",), ROWS: ("PX", "ACC"), MFMA: ("CT", "ACC", "CIT", "POOL", "WH", "DMA", "prepped"),
                IMG: ("CT", "TPW", "POOL", "WP", "gap", "tile_store", "prepped"), CHAIN: ("S", "C_IN", "C_OUT", "POST", "LIN"),
                WGRAD_MFMA: ("CT", "PQ", "ending"), WGRAD_IMG: ("S", "C_IN", "C_OUT", "ending"), WGRAD_CONV1: ("ending",),
                WGRAD_VEC: ("slabs", "ending", "accumulate")}


def forms_table():
    """the table of DESIGN.md section 3b: per op and kernel family the values each parameter of the form takes over the reachable forms (not
    every combination is reachable: the count says how many are), and the smallest reaching shape of the sweep"""
    reach = reachable_forms()
    rows = ["| op | kernel family | parameters of the form and the values reached | forms | smallest shape of the sweep (n x c_in x h x w -> c_out) |",
            "|---|---|---|---|---|"]
    for op, fam in sorted({f[:2] for f in reach}):
        fs = sorted(f for f in reach if f[:2] == (op, fam))
        c = min((reach[f] for f in fs), key=_size)
        if fam == CHAIN:
            var = "(S, C_IN, C_OUT, POST, LIN) in " + " ".join(str(f[2:]).replace(" ", "") for f in fs)
        elif fam == WGRAD_IMG:
            var = "(S, C_IN, C_OUT) in " + " ".join(sorted({str(f[2:5]).replace(" ", "") for f in fs})) + "; ending " + "/".join(
                str(v) for v in sorted({f[5] for f in fs}))
        else:
            var = "; ".join(f"{name} " + "/".join(str(v) for v in sorted({f[2 + i] for f in fs})) for i, name in enumerate(_FORM_PARAMS[fam]))
        rows.append(f"| {OP_NAMES[op]} | {FAMILY_NAMES[fam]} | {var} | {len(fs)} | {c[1]} x {c[2]} x {c[3]} x {c[4]} -> {c[5]} |")
    return "\n".join(rows)


if __name__ == "__main__":      # prints what GENERATED_CASES lacks, then the table of forms of DESIGN.md section 3b
    have, reach = cases_by_form(), reachable_forms()
    for f in sorted(reach):
        if f not in have:
            print(f"    {reach[f]},   # {form_name(f)}")
    print(f"{len(reach)} forms reachable, {len(have)} reached by the case table; per op: " +
          ", ".join(f"{OP_NAMES[op]} {sum(1 for f in reach if f[0] == op)}" for op in range(5)))
    print(forms_table())
