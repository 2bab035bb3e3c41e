"""th_debug_linear_fwd_ex_plan (csrc/gemm.hip: the host function th_linear_fwd_ex itself launches from) without a GPU: its ABI, that the
sub-tiles of every grid cover H exactly once, the workgroup bound of the sub-tile forms, and where the 16 x 16 form stays."""
import ctypes as C

import numpy as np

from taper_amd._lib import INCLUDE, hip, parse_header

FIELDS = ("one_launch", "rm", "rn", "waves", "cpw", "grid_x", "grid_y", "xcd")
CHOSEN_B64 = (8, 8, 16, 1)      # (64, 784, 128): sub-tile rows, columns, waves, chunks per wave (profiles/mlp_fwd_subtiles.md)


def plan(batch, inf, outf, subtiles=1):
    out = (C.c_int * 8)()
    assert hip.th_debug_linear_fwd_ex_plan(batch, inf, outf, subtiles, out) == 0, hip.th_last_error()
    return dict(zip(FIELDS, out))


def test_hook_is_a_debug_symbol_and_checks_its_arguments():
    assert "th_debug_linear_fwd_ex_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_linear_fwd_ex_plan" not in parse_header(INCLUDE / "taper_hip.h")
    assert "th_linear_fwd_ex_set_subtiles" in parse_header(INCLUDE / "taper_hip.h")
    out = (C.c_int * 8)()
    for bad in [(0, 784, 128), (64, 0, 128), (64, 784, 0), (-1, 784, 128)]:
        assert hip.th_debug_linear_fwd_ex_plan(*bad, 1, out) != 0 and b"th_debug_linear_fwd_ex_plan" in hip.th_last_error(), bad
    assert hip.th_debug_linear_fwd_ex_plan(64, 784, 128, 1, None) != 0
    assert hip.th_linear_fwd_ex_set_subtiles(None, 1) != 0


def tile_of_block(p, bx, by):
    """sgemm_small16_tick's workgroup-to-(sub-)tile map: linear, or -- p['xcd'] -- block b to the (b % 8)-th 32 x 32 block of H"""
    if not p["xcd"]:
        return by, bx
    sbm, sbn = 32 // p["rm"], 32 // p["rn"]
    b = bx + p["grid_x"] * by
    q, j = b & 7, b >> 3
    return sbm * (q >> 2) + j // sbn, sbn * (q & 3) + j % sbn


def test_subtiles_cover_h_exactly_once():
    """every m, n in 1 .. 130 at k = 784: each element of H belongs to exactly one workgroup of the grid's tile rows"""
    smaller = 0
    for m in range(1, 131):
        for n in range(1, 131):
            p = plan(m, 784, n)
            assert p["one_launch"] == 1 and (p["rm"], p["rn"]) in ((8, 8), (16, 16)) and p["grid_y"] >= 2, (m, n, p)
            hits = np.zeros((m, n), np.int32)
            tiles = set()
            for by in range(p["grid_y"] - 1):
                for bx in range(p["grid_x"]):
                    tm, tn = tile_of_block(p, bx, by)
                    tiles.add((tm, tn))
                    hits[tm * p["rm"]:(tm + 1) * p["rm"], tn * p["rn"]:(tn + 1) * p["rn"]] += 1
                    assert tm * p["rm"] < m and tn * p["rn"] < n, (m, n, p, bx, by)     # no workgroup without an element: its row clamp relies on it
            assert (hits == 1).all(), (m, n, p)
            wgs = p["grid_x"] * (p["grid_y"] - 1)
            assert len(tiles) == wgs
            if (p["rm"], p["rn"]) != (16, 16):
                smaller += 1
                assert wgs <= 256 and p["waves"] * p["cpw"] == 16, (m, n, p)
            assert p["xcd"] == int(p["grid_x"] * p["rn"] == 128 and (p["grid_y"] - 1) * p["rm"] == 64), (m, n, p)
    assert smaller > 0


def test_where_the_16x16_form_stays():
    for shape in [(64, 784, 128), (128, 784, 128), (16, 256, 16), (7, 260, 9)]:
        off = plan(*shape, subtiles=0)
        assert (off["rm"], off["rn"], off["waves"], off["cpw"]) == (16, 16, 16, 1), shape       # the switch off: today's launch
        assert off["grid_x"] == -(-shape[2] // 16) and off["grid_y"] == -(-shape[0] // 16) + 1
    assert plan(64, 784, 128, 0)["xcd"] == 1 and plan(128, 784, 128, 0)["xcd"] == 0
    for k in (1, 16, 100, 255):                                                               # k < 256: the 4-wave 16 x 16 instance
        p = plan(64, k, 128)
        assert (p["rm"], p["rn"], p["waves"], p["cpw"]) == (16, 16, 4, 1), k
    for shape in [(64, 1028, 128), (64, 2044, 128), (65, 784, 128), (128, 784, 128), (64, 784, 132), (256, 784, 128)]:   # outside what was measured
        p = plan(*shape)
        assert p["one_launch"] == 1 and (p["rm"], p["rn"]) == (16, 16), shape
    assert plan(64, 4096, 128)["one_launch"] == 0                                             # deep K on few tiles: th_linear_fwd's K slices


def test_the_measured_shapes():
    p = plan(64, 784, 128)
    assert (p["rm"], p["rn"], p["waves"], p["cpw"]) == CHOSEN_B64 and p["xcd"] == 1
    assert p["grid_x"] == 128 // p["rn"] and p["grid_y"] == 64 // p["rm"] + 1
    q = plan(128, 784, 128)                     # batch 128: not measured, the 16 x 16 form
    assert (q["rm"], q["rn"], q["waves"], q["grid_x"], q["grid_y"], q["xcd"]) == (16, 16, 16, 8, 9, 0)
