"""th_debug_conv1x1_exact_plan (csrc/conv_pw_plan.h: the host functions th_conv1x1_exact_fwd / _bwd_input / _bwd_weight themselves launch
from) without a GPU: its ABI, the plan's invariants over the whole sweep, the coverage of the GPU case table of
tests/test_gpu_conv_pw_forms.py, the thresholds of the plans from both sides, the refusals, and tests/conv_pw_ref.py's numpy reference against
torch's strided 1x1 convolution and its autograd."""
import ctypes as C

import numpy as np
import pytest

from taper_amd._lib import INCLUDE, hip, parse_header
from tests import conv_pw_ref as R
from tests.conv_pw_ref import BWD_INPUT, BWD_WEIGHT, FWD, R_COLSUM, R_COLSUM_ACCUM, R_SCATTER, R_SLAB_SUM, _c, plan


def test_hook_is_a_debug_symbol_and_checks_its_arguments():
    for name in ("th_debug_conv1x1_exact_plan", "th_debug_last_conv_pw_config"):
        assert name in parse_header(INCLUDE / "taper_hip_debug.h")
        assert name not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    for name in R.ENTRY_POINTS:
        assert name in parse_header(INCLUDE / "taper_hip.h")
    out = (C.c_int * len(R.PLAN_FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = (0, 4, 8, 14, 14, 16, 2, 0, 3, 0, 0)
    assert hip.th_debug_conv1x1_exact_plan(*good, ptr) == 0
    for i, v, word in ((0, 3, b"op"), (0, -1, b"op"), (1, 0, b"geometry"), (2, 0, b"geometry"), (3, 0, b"geometry"), (4, -3, b"geometry"),
                       (5, 0, b"geometry"), (6, 0, b"stride"), (6, 3, b"stride"), (7, 2, b"weight_layout"), (7, -1, b"weight_layout"),
                       (8, 4, b"relu_bias"), (8, -1, b"relu_bias"), (9, 2, b"accumulate"), (9, 1, b"accumulate"), (10, 2, b"w_misalign_bytes"),
                       (10, 16, b"w_misalign_bytes")):
        bad = list(good)
        bad[i] = v
        assert hip.th_debug_conv1x1_exact_plan(*bad, ptr) != 0, bad
        err = hip.th_last_error()
        assert b"th_debug_conv1x1_exact_plan" in err and word in err, (bad, err)
    assert hip.th_debug_conv1x1_exact_plan(1, 4, 8, 14, 14, 16, 1, 0, 3, 0, 0, ptr) != 0 and b"relu_bias" in hip.th_last_error()   # a gradient has neither
    assert hip.th_debug_conv1x1_exact_plan(*good, None) != 0 and b"null output" in hip.th_last_error()
    # the struct and the field list of tests/conv_pw_ref.py are the same length: the last fields are h_out, w_out
    p = plan(FWD, 2, 3, 5, 6, 4, 2)
    assert (p["op"], p["stride"], p["h_out"], p["w_out"]) == (0, 2, 3, 3)
    assert plan(BWD_WEIGHT, 2, 3, 6, 1, 4, 2)["h_out"] == 3 and plan(BWD_INPUT, 1, 1, 5, 6, 1, 1)["w_out"] == 6


def test_plan_invariants_over_the_sweep():
    """tests/conv_pw_ref.py: violations() on every plan of the sweep -- tiles that cover the flat pixel axis, every grid dimension at least 1,
    within the device limit and equal to the tile counts, the images behind a tile's descriptor counted right and below 2 GiB, LDS as the
    kernels declare it, G <= min(pixel blocks, 512), slab_sum_kernel only where it may run"""
    bad = R.sweep()[1]
    assert not bad, f"{len(bad)} broken invariants, e.g. " + "; ".join(f"{c}: {b}" for c, b in bad[:5])


def test_case_table_covers_every_reachable_form():
    """The condition of the GPU module: its case table reaches every form th_debug_conv1x1_exact_plan reports anywhere on the sweep.

    What the sweep finds (42 forms): forward 3 CT x 2 strides = 6; input gradient 3 CT x 2 strides x accumulate = 12; weight gradient
    3 CT x 2 strides x 4 reduce endings = 24."""
    reach, have = R.reachable_forms(), R.cases_by_form()
    missing = sorted(f for f in reach if f not in have)
    assert not missing, "forms no GPU case reaches:\n" + "\n".join(f"  {R.form_name(f)}  e.g. {reach[f]}" for f in missing)
    assert len(reach) == 42, len(reach)      # (a retuned threshold that adds or removes a form says so here)
    assert [sum(1 for f in reach if f[0] == op) for op in range(3)] == [6, 12, 24]
    assert not any(f[1] == 0 for f in reach)      # nothing on the sweep is refused
    for c in R.CASES:      # every case stands inside the exactness argument of tests/conv_pw_ref.py
        n, c_in, h, w, c_out, s = c[1:7]
        ho, wo = R.out_hw(h, w, s)
        assert 16 * max(c_in, c_out) + 16 < 2 ** 24 and 16 * n * ho * wo + 8 < 2 ** 24, c
    assert len(set(R.CASES)) == len(R.CASES)


def _is(case, **want):
    p = plan(*case)
    assert {k: p[k] for k in want} == want, (case, R.form_name(R.form_of(*case)), p)


def test_named_rows_take_the_paths_their_comments_name():
    for op in (FWD, BWD_INPUT):
        _is(_c(op, 3, 9, 33, 20, 17, 1), tiles=16, grid_x=16, grid_y=1, span=2)      # 1980 pixels: an image is 5.2 tiles
        _is(_c(op, 3, 9, 33, 20, 17, 2), tiles=4, span=2, h_out=17, w_out=10)              # 510 pixels
        _is(_c(op, 3, 9, 1, 1, 17, 2), tiles=1, span=3)
        _is(_c(op, 128, 3, 1, 1, 5, 1), tiles=1, span=128)                                # 128 one-pixel images: one full tile
        _is(_c(op, 129, 3, 1, 1, 5, 1), tiles=2, span=128)                                # and one image past it
        _is(_c(op, 15, 8, 5, 6, 16, 2), tiles=2, span=15)                                 # 9 pixels an image: 14.2 images a tile
        _is(_c(op, 2, 3, 3, 300, 5, 1), tiles=15, span=2)
    _is(_c(BWD_WEIGHT, 3, 33, 6, 5, 17, 1), grid_y=2, co_ld=32, grid_z=1, reduce=R_SCATTER)
    for s, (n16, n15) in ((1, (65, 63)), (2, (214, 213))):
        _is(_c(BWD_WEIGHT, n16, 8, 5, 6, 16, s), tiles=16, G=16, reduce=R_SLAB_SUM)
        _is(_c(BWD_WEIGHT, n15, 8, 5, 6, 16, s), tiles=15, G=15, reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 3, 8, 6, 5, 16, 1, w_off=4), reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 3, 8, 6, 5, 16, 1, acc=1, w_off=4), reduce=R_COLSUM_ACCUM)
    _is(_c(BWD_WEIGHT, 3, 9, 6, 5, 17, 1, layout=1), reduce=R_SCATTER)
    for c in R.NAMED_CASES:
        assert c in R.CASES


def test_threshold_ct_4_to_2_below_384_workgroup_slots():
    """64 channels per workgroup (CT 4) from 384 (tile, 64-channel block) slots, 32 (CT 2) below -- conv3x3_mfma_plan's rule, here for the
    forward (output channels) and the input gradient (input channels): 8 x 8 planes are half a tile"""
    for op, ci, co in ((FWD, 8, 128), (BWD_INPUT, 128, 8)):
        _is(_c(op, 382, ci, 8, 8, co), ct=2, grid_x=191, grid_y=4)
        _is(_c(op, 383, ci, 8, 8, co), ct=4, grid_x=192, grid_y=2)
    _is(_c(FWD, 766, 8, 8, 8, 64), ct=2, grid_x=383)
    _is(_c(FWD, 767, 8, 8, 8, 64), ct=4, grid_x=384)
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 64), ct=4)      # the weight gradient goes by the channel tiles alone
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 63), ct=4, co_ld=64)
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 48), ct=2, co_ld=64, grid_z=2)
    _is(_c(BWD_WEIGHT, 256, 64, 14, 14, 256), G=64, grid_y=2, grid_z=4)      # two workgroups per CU: 512 / (2 x 4)


def test_refusals_of_the_plan():
    """what a buffer descriptor with 32-bit byte offsets cannot address is refused (2), and so are 2^31 output pixels and more (1); a refused
    plan holds no slabs: the entry point returns before it takes workspace"""
    # forward: the two images a 128-pixel tile of a 64 x 64 plane can touch hold 2 x c_in x 16 KiB
    assert plan(FWD, 4, 65536, 64, 64, 8)["refused"] == 2 and plan(FWD, 4, 65535, 64, 64, 8)["refused"] == 0
    assert plan(FWD, 1, 65536, 64, 64, 8)["refused"] == 0      # one image alone: 1 GiB
    # input gradient: the descriptor lies on gy (c_out x h_out x w_out an image)
    assert plan(BWD_INPUT, 4, 8, 64, 64, 65536)["refused"] == 2 and plan(BWD_INPUT, 4, 8, 64, 64, 65536, 2)["refused"] == 0
    assert plan(BWD_INPUT, 4, 65536, 64, 64, 8)["refused"] == 0
    # weight gradient: the whole maps
    assert plan(BWD_WEIGHT, 2048, 64, 64, 64, 8)["refused"] == 2 and plan(BWD_WEIGHT, 2047, 64, 64, 64, 8)["refused"] == 0
    assert plan(BWD_WEIGHT, 2048, 8, 64, 64, 64, 2)["refused"] == 0 and plan(BWD_WEIGHT, 2048, 8, 64, 64, 256, 2)["refused"] == 2   # gy at stride 2
    assert plan(FWD, 2048, 64, 64, 64, 8)["refused"] == 0 and plan(BWD_INPUT, 2048, 64, 64, 64, 8)["refused"] == 0
    # 2^31 output pixels
    for op in range(3):
        p = plan(op, 32768, 1, 256, 256, 1)
        assert p["refused"] == 1 and p["slabs"] == 0 and p["G"] == 0, p
    for op in range(3):
        p = plan(op, 32768, 1, 256, 256, 1, 2)
        assert p["refused"] == (0 if op < 2 else 2), p       # a quarter of the pixels; the weight gradient's x is 8 GiB
    for case in ((BWD_WEIGHT, 2048, 64, 64, 64, 8), (FWD, 4, 65536, 64, 64, 8)):
        p = plan(*case)
        assert p["refused"] == 2 and p["slabs"] == 0 and p["G"] == 0, p


# ------------------------------------------------------------------------------------------------ the reference against torch
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
from tests import conv_pw_ref as R
n, c_in, c_out = 3, 9, 17
for h, w in ((1, 1), (2, 2), (5, 6), (7, 2), (33, 20)):
    for s in (1, 2):
        x, wt, bias, gy = R.operands(R._c(R.FWD, n, c_in, h, w, c_out, s))
        for layout in (0, 1):
            w_std = wt if layout == 1 else np.ascontiguousarray(wt.reshape(c_in, c_out).T).reshape(c_out, c_in, 1, 1)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            wtt = torch.tensor(w_std, dtype=torch.float64, requires_grad=True)
            y = torch.nn.functional.conv2d(xt, wtt, torch.tensor(bias, dtype=torch.float64), stride=s)
            assert tuple(y.shape[2:]) == R.out_hw(h, w, s)
            bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
            eq = lambda a, b: np.testing.assert_array_equal(bits(a), bits(b))
            eq(R.forward(x, wt, bias, s, layout, 0), y.detach().numpy())
            eq(R.forward(x, wt, bias, s, layout, 1), torch.relu(y).detach().numpy())
            eq(R.forward(x, wt, None, s, layout, 0), y.detach().numpy() - bias[None, :, None, None])
            # the NaN the GPU tests put into the skipped pixels never reaches the reference
            eq(R.forward(R.poison_skipped(x, s), wt, bias, s, layout, 0), y.detach().numpy())
            (y * torch.tensor(gy, dtype=torch.float64)).sum().backward()
            eq(R.input_grad(gy, wt, c_in, h, w, s, layout), xt.grad.numpy())
            gw = wtt.grad.numpy().astype(np.float32)      # [co][ci][1][1]
            gw_mem = gw if layout == 1 else np.ascontiguousarray(gw.reshape(c_out, c_in).T).reshape(c_out, c_in, 1, 1)
            eq(R.weight_grad(x, gy, s, layout), gw_mem)
            eq(R.weight_grad(R.poison_skipped(x, s), gy, s, layout), gw_mem)
print("identities hold")
"""


def test_reference_equals_torch_on_bits():
    """tests/conv_pw_ref.py's three functions against torch.nn.functional.conv2d(stride=s) and its autograd on the CPU, on the integer data of
    the GPU tests and on bits (the uint32 view: the +0.0 of the unread input-gradient pixels included), for both strides over planes 1x1, 2x2,
    5x6, 7x2 and 33x20 with 3 images and 9 -> 17 channels (layout 1 is torch's filter; layout 0 reads the same buffer as [c_in][c_out]).  In a
    process of its own: torch brings its own HIP runtime, which must not share a process with libtaper_hip.so."""
    import importlib.util
    import subprocess
    import sys
    from pathlib import Path
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK], cwd=Path(__file__).resolve().parent.parent, capture_output=True, text=True)
    assert r.returncode == 0 and "identities hold" in r.stdout, r.stdout + r.stderr
