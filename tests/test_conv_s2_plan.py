"""th_debug_conv3x3_s2_plan (csrc/conv_s2_plan.h: the host functions th_conv3x3_s2_fwd / _bwd_input / _bwd_weight themselves launch from)
without a GPU: its ABI, the plan's invariants over the whole sweep, the coverage of the GPU case table of tests/test_gpu_conv_s2_forms.py, the
thresholds of the plans from both sides, and tests/conv_s2_ref.py's numpy reference against torch's strided convolution and its autograd."""
import ctypes as C

import numpy as np
import pytest

from taper_amd._lib import INCLUDE, hip, parse_header
from tests import conv_s2_ref as R
from tests.conv_s2_ref import BWD_INPUT, BWD_WEIGHT, FWD, R_COLSUM, R_COLSUM_ACCUM, R_SCATTER, R_SLAB_SUM, _c, plan


def test_hook_is_a_debug_symbol_and_checks_its_arguments():
    for name in ("th_debug_conv3x3_s2_plan", "th_debug_last_conv_s2_config"):
        assert name in parse_header(INCLUDE / "taper_hip_debug.h")
        assert name not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    for name in R.ENTRY_POINTS:
        assert name in parse_header(INCLUDE / "taper_hip.h")
    out = (C.c_int * len(R.PLAN_FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = (0, 4, 8, 14, 14, 16, 0, 3, 0, 0)
    assert hip.th_debug_conv3x3_s2_plan(*good, ptr) == 0
    for i, v, word in ((0, 3, b"op"), (0, -1, b"op"), (1, 0, b"geometry"), (2, 0, b"geometry"), (3, 0, b"geometry"), (4, -3, b"geometry"),
                       (5, 0, b"geometry"), (6, 2, b"weight_layout"), (6, -1, b"weight_layout"), (7, 4, b"relu_bias"), (7, -1, b"relu_bias"),
                       (8, 2, b"accumulate"), (8, 1, b"accumulate"), (9, 2, b"w_misalign_bytes"), (9, 16, b"w_misalign_bytes")):
        bad = list(good)
        bad[i] = v
        assert hip.th_debug_conv3x3_s2_plan(*bad, ptr) != 0, bad
        err = hip.th_last_error()
        assert b"th_debug_conv3x3_s2_plan" in err and word in err, (bad, err)
    assert hip.th_debug_conv3x3_s2_plan(1, 4, 8, 14, 14, 16, 0, 3, 0, 0, ptr) != 0 and b"relu_bias" in hip.th_last_error()   # a gradient has neither
    assert hip.th_debug_conv3x3_s2_plan(*good, None) != 0 and b"null output" in hip.th_last_error()
    # the struct and the field list of tests/conv_s2_ref.py are the same length: the last fields are h_out, w_out
    p = plan(FWD, 2, 3, 5, 6, 4)
    assert (p["op"], p["h_out"], p["w_out"]) == (0, 3, 3) and plan(BWD_WEIGHT, 2, 3, 6, 1, 4)["h_out"] == 3 and plan(BWD_INPUT, 1, 1, 1, 1, 1)["w_out"] == 1


def test_plan_invariants_over_the_sweep():
    """tests/conv_s2_ref.py: violations() on every plan of the sweep -- LDS at or below what the launch requests, at most 128 pixels per
    workgroup, tiles that cover the output, every grid dimension at least 1 and equal to the tile counts, staged chunks within what the
    threads hold, G <= min(n_pb, 512), slab_sum_kernel only where it may run"""
    bad = R.sweep()[1]
    assert not bad, f"{len(bad)} broken invariants, e.g. " + "; ".join(f"{c}: {b}" for c, b in bad[:5])


def test_case_table_covers_every_reachable_form():
    """The condition of the GPU module: its case table reaches every form th_debug_conv3x3_s2_plan reports anywhere on the sweep.

    What the sweep finds (42 forms): forward 3 CT x with / without column blocks = 6; input gradient 3 CT x accumulate x column blocks = 12;
    weight gradient 3 CT x 4 reduce endings x column blocks = 24."""
    reach, have = R.reachable_forms(), R.cases_by_form()
    missing = sorted(f for f in reach if f not in have)
    assert not missing, "forms no GPU case reaches:\n" + "\n".join(f"  {R.form_name(f)}  e.g. {reach[f]}" for f in missing)
    assert len(reach) == 42, len(reach)      # (a retuned threshold that adds or removes a form says so here)
    assert [sum(1 for f in reach if f[0] == op) for op in range(3)] == [6, 12, 24]
    assert not any(f[1] == 0 for f in reach)      # nothing on the sweep is refused
    for c in R.CASES:      # every case stands inside the exactness argument of tests/conv_s2_ref.py
        n, c_in, h, w, c_out = c[1:6]
        ho, wo = R.out_hw(h, w)
        assert 16 * 9 * max(c_in, c_out) + 16 < 2 ** 24 and 16 * n * ho * wo + 8 < 2 ** 24, c
    assert len(set(R.CASES)) == len(R.CASES)


def _is(case, **want):
    p = plan(*case)
    assert {k: p[k] for k in want} == want, (case, R.form_name(R.form_of(*case)), p)


def test_named_rows_take_the_paths_their_comments_name():
    for op in (FWD, BWD_INPUT):      # 17 output rows in bands of 6, 6 and 5; three images in groups of two
        _is(_c(op, 3, 9, 33, 20, 17), rows_t=6, bands=3, cols_t=10, cblks=1, img_t=2, grid_x=6)
    _is(_c(BWD_WEIGHT, 3, 9, 33, 20, 17), rows_t=6, bands=3, cols_t=10, img_t=1, n_pb=9)   # (2 x 13 x 21 floats of a channel's band are over 512)
    for op in range(3):
        _is(_c(op, 3, 9, 1, 1, 17), rows_t=1, cols_t=1, img_t=3, grid_x=1)
        _is(_c(op, 3, 9, 7, 2, 17), rows_t=4, cols_t=1, bands=1)
    _is(_c(FWD, 15, 8, 5, 6, 16), img_t=14, grid_x=2)                                       # 128 // 9 images per group: one past it
    _is(_c(BWD_INPUT, 15, 8, 5, 6, 16), img_t=14, grid_x=2)
    _is(_c(BWD_WEIGHT, 15, 8, 5, 6, 16), img_t=10, n_pb=2)                                  # 512 // 49 floats of a channel's band
    _is(_c(FWD, 2, 3, 4, 300, 5), cols_t=75, cblks=2, rows_t=1, bands=2)
    _is(_c(BWD_INPUT, 2, 3, 3, 299, 5), cols_t=75, cblks=2)
    _is(_c(BWD_WEIGHT, 2, 3, 4, 300, 5), cols_t=50, cblks=3)
    _is(_c(BWD_WEIGHT, 1, 1, 3, 255, 16), cols_t=64, cblks=2)                               # w_out = 128: one block forward, two here
    _is(_c(FWD, 1, 1, 3, 255, 16), cols_t=128, cblks=1, img_t=1)
    _is(_c(BWD_WEIGHT, 16, 8, 33, 20, 16), G=34, n_pb=34, reduce=R_SLAB_SUM)
    _is(_c(BWD_WEIGHT, 15, 8, 16, 20, 16), G=15, n_pb=15, reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 3, 8, 6, 5, 16, w_off=4), reduce=R_COLSUM)
    _is(_c(BWD_WEIGHT, 3, 8, 6, 5, 16, acc=1, w_off=4), reduce=R_COLSUM_ACCUM)
    _is(_c(BWD_WEIGHT, 3, 9, 6, 5, 17), reduce=R_SCATTER, co_ld=32, grid_y=1, grid_z=1)
    _is(_c(BWD_WEIGHT, 3, 9, 6, 5, 17, layout=1), reduce=R_SCATTER)
    for c in R.NAMED_CASES:
        assert c in R.CASES


def test_threshold_ct_4_to_2_below_384_workgroup_slots():
    """64 channels per workgroup (CT 4) from 384 (tile, 64-channel block) slots, 32 (CT 2) below -- conv3x3_mfma_plan's rule, here for
    the forward (output channels) and the input gradient (input channels): 8 x 8 planes have 16 outputs, 8 images a tile"""
    for op, ci, co in ((FWD, 8, 128), (BWD_INPUT, 128, 8)):
        _is(_c(op, 1528, ci, 8, 8, co), ct=2, grid_x=191, grid_y=4)
        _is(_c(op, 1529, ci, 8, 8, co), ct=4, grid_x=192, grid_y=2)
    _is(_c(FWD, 8 * 383, 8, 8, 8, 64), ct=2)
    _is(_c(FWD, 8 * 384, 8, 8, 8, 64), ct=4)
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 64), ct=4)      # the weight gradient goes by the channel tiles alone
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 63), ct=4, co_ld=64)
    _is(_c(BWD_WEIGHT, 1, 8, 8, 8, 48), ct=2, co_ld=64, grid_z=2)


def test_refusals_of_the_plan():
    """the weight gradient's buffer descriptors hold maps below 2 GiB: the plan says so, and nothing else is refused"""
    assert plan(BWD_WEIGHT, 2048, 64, 64, 64, 8)["refused"] == 2      # x: 2 GiB
    assert plan(BWD_WEIGHT, 2047, 64, 64, 64, 8)["refused"] == 0
    assert plan(FWD, 2048, 64, 64, 64, 8)["refused"] == 0 and plan(BWD_INPUT, 2048, 64, 64, 64, 8)["refused"] == 0


# ------------------------------------------------------------------------------------------------ the reference against torch
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
from tests import conv_s2_ref as R
for n, c_in, h, w, c_out in ((2, 3, 5, 6, 4), (2, 3, 6, 5, 4), (1, 8, 1, 1, 5), (3, 1, 2, 2, 2), (2, 9, 7, 2, 17), (1, 2, 8, 8, 3)):
    x, wt, bias, gy = R.operands(R._c(R.FWD, n, c_in, h, w, c_out))
    k = 9 * c_in
    for layout in (0, 1):
        w_std = wt if layout == 1 else np.ascontiguousarray(wt.reshape(k, c_out).T).reshape(c_out, c_in, 3, 3)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        wtt = torch.tensor(w_std, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(xt, wtt, torch.tensor(bias, dtype=torch.float64), stride=2, padding=1)
        assert tuple(y.shape[2:]) == R.out_hw(h, w)
        np.testing.assert_array_equal(R.forward(x, wt, bias, layout, 0), y.detach().numpy().astype(np.float32))
        np.testing.assert_array_equal(R.forward(x, wt, bias, layout, 1), torch.relu(y).detach().numpy().astype(np.float32))
        np.testing.assert_array_equal(R.forward(x, wt, None, layout, 0), (y.detach().numpy() - bias[None, :, None, None]).astype(np.float32))
        (y * torch.tensor(gy, dtype=torch.float64)).sum().backward()
        np.testing.assert_array_equal(R.input_grad(gy, wt, c_in, h, w, layout), xt.grad.numpy().astype(np.float32))
        gw = wtt.grad.numpy().astype(np.float32)      # [co][ci][kh][kw]
        gw_mem = gw if layout == 1 else np.ascontiguousarray(gw.reshape(c_out, k).T).reshape(c_out, c_in, 3, 3)
        np.testing.assert_array_equal(R.weight_grad(x, gy, layout), gw_mem)
print("identities hold")
"""


def test_reference_equals_torch_on_bits():
    """tests/conv_s2_ref.py's three identities against torch.nn.functional.conv2d(stride=2, padding=1) and its autograd on the CPU, on the
    integer data of the GPU tests, over odd, even and one-pixel planes (layout 1 is torch's filter; layout 0 reads the same buffer as
    [9 c_in][c_out]).  In a process of its own: torch brings its own HIP runtime, which must not share a process with libtaper_hip.so."""
    import importlib.util
    import subprocess
    import sys
    from pathlib import Path
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch is not installed")
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK], cwd=Path(__file__).resolve().parent.parent, capture_output=True, text=True)
    assert r.returncode == 0 and "identities hold" in r.stdout, r.stdout + r.stderr
