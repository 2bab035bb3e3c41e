"""Post-training quantization's boundary without a GPU: the C ABI declarations (include/taper_hip.h, include/taper_host.h), the
Python face (Module.quantize -> QuantizedModule), the invariants of the quantized Linear's launch plan (th_debug_qlinear_plan, the
host function the launch consumes) and what the case table of tests/test_gpu_qlinear.py covers according to that plan."""
import inspect
import itertools

import pytest


def test_kernel_entry_points_are_declared_and_exported():
    from taper_amd._lib import HIP_PROTOS
    for name, nargs in (("th_linear_q8_fwd", 11), ("th_linear_h16_fwd", 9), ("th_dequantize_multi", 3), ("th_qlinear_stream_max_batch", 0),
                        ("th_debug_qlinear_plan", 7)):
        assert name in HIP_PROTOS and len(HIP_PROTOS[name][1]) == nargs, name


def test_host_entry_points_are_declared_and_exported():
    from taper_amd._lib import HOST_PROTOS
    for name, nargs in (("tp_module_quantize", 4), ("tp_qmodule_forward", 3), ("tp_qmodule_storage_bytes", 2), ("tp_qmodule_num_tensors", 2),
                        ("tp_qmodule_tensor_len", 3), ("tp_qmodule_tensor", 5), ("tp_qmodule_free", 1)):
        assert name in HOST_PROTOS and len(HOST_PROTOS[name][1]) == nargs, name


def test_qtensor_struct_matches_the_header():
    import ctypes as C

    from taper_amd import hip
    assert C.sizeof(hip.QTensor) == 40 and hip.QTensor.n.offset == 24 and hip.QTensor.qtype.offset == 32


def test_python_face():
    import taper_amd as T
    assert callable(T.Module.quantize) and T.QuantizedModule.__call__ is T.QuantizedModule.forward
    assert list(inspect.signature(T.Module.quantize).parameters) == ["self", "qtype", "enabled"]
    assert set(T.QuantizedModule.QTYPES) == {"int8", "float16", "int4", "bfloat16", "nf4"}
    for meth in ("forward", "storage_bytes", "tensors"):
        assert callable(getattr(T.QuantizedModule, meth))


def test_unknown_qtype_is_refused_before_the_device():
    import taper_amd as T
    m = T.Module.__new__(T.Module)
    m._h = None
    with pytest.raises(T.TaperError, match="unknown qtype"):
        m.quantize("int2")


# ---------------------------------------------------------------- the quantized Linear's launch plan
def test_plan_query_is_a_debug_hook_and_refuses_nonsense():
    from taper_amd._lib import INCLUDE, hip, parse_header
    assert "th_debug_qlinear_plan" in parse_header(INCLUDE / "taper_hip_debug.h")
    assert "th_debug_qlinear_plan" not in parse_header(INCLUDE / "taper_hip.h")      # not part of the drop-in boundary
    import ctypes as C
    out = (C.c_int * 8)()
    ptr = C.cast(out, C.c_void_p)
    assert hip.th_debug_qlinear_plan(0, 1, 128, 10, 0, 0, ptr) == 0
    for bad in ((2, 1, 128, 10, 0, 0), (-1, 1, 128, 10, 0, 0), (0, 0, 128, 10, 0, 0), (0, 1, 0, 10, 0, 0), (1, 1, 128, 0, 0, 0),
                (1, 1, 128, 10, -4, 0)):
        assert hip.th_debug_qlinear_plan(*bad, ptr) != 0 and b"th_debug_qlinear_plan" in hip.th_last_error(), bad
    assert hip.th_debug_qlinear_plan(0, 1, 128, 10, 0, 0, None) != 0


def test_plan_invariants_over_a_grid():
    from tests.test_gpu_qlinear import LOAD, max_batch, plan
    M = max_batch()
    Ks = [1, 7, 8, 15, 16, 17, 100, 511, 512, 513, 784, 1000, 1023, 1024, 1025, 1027, 2048, 2051, 2560, 3000, 4096, 5120, 8192, 100003]
    Ns = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 1000, 4096, 5472, 16383, 16384, 16400, 100000]
    offs = [(0, 0), (4, 0), (0, 2), (12, 14), (16, 32), (0, 16), (20, 0)]
    for qtype, B, K, N in itertools.product(("int8", "f16"), list(range(1, 2 * M + 3)) + [64, 257], Ks, Ns):
        E = LOAD[qtype]
        for xo, wo in offs if (K, N) in ((1024, 17), (100, 5), (2051, 65)) or B == 1 and N == 17 else offs[:1]:
            p = plan(qtype, B, K, N, xo, wo)
            tag = (qtype, B, K, N, xo, wo, p)
            assert p["stream"] == (1 if B <= M else 0), tag
            if not p["stream"]:
                assert not any(p[f] for f in p if f != "stream"), tag
                continue
            assert p["vec"] == (1 if K % E == 0 and xo % 16 == 0 and wo % 16 == 0 else 0), tag
            assert p["bt"] in (1, 2, 4, 8) and p["bt"] >= B and (p["bt"] == 1 or p["bt"] // 2 < B), tag
            assert p["kslice"] > 0 and p["kslice"] % (64 * E) == 0, tag
            assert (p["S"] - 1) * p["kslice"] < K <= p["S"] * p["kslice"], tag
            assert p["blocks_n"] == -(-N // 16) and p["steps"] == -(-K // (64 * E)), tag
            assert 1 <= p["S"] <= p["want"] <= p["steps"], tag


def _table():
    from tests.test_gpu_qlinear import CASES, plan
    return [(c, plan(*c)) for c in CASES]


def test_case_table_is_well_formed():
    from tests.test_gpu_qlinear import CASES, CODE
    assert len(set(CASES)) == len(CASES)
    for qtype, B, K, N, xo, wo in CASES:
        assert qtype in CODE and B >= 1 and 1 <= K <= 8192 and N >= 1      # K <= 8192: the exact-arithmetic bound 4 * 128 * K + 100 < 2^24
        assert 0 <= xo < 16 and xo % 4 == 0 and 0 <= wo < 16 and wo % CODE[qtype] == 0


def test_case_table_covers_every_kernel_instance():
    """all 32 cells of (codec, batch tile, vector / element loads, one slice / K split)"""
    have = {(c[0], p["bt"], p["vec"], p["S"] > 1) for c, p in _table() if p["stream"]}
    want = set(itertools.product(("int8", "f16"), (1, 2, 4, 8), (0, 1), (False, True)))
    assert want - have == set() and len(want) == 32, sorted(want - have)


def test_case_table_covers_the_edges():
    from tests.test_gpu_qlinear import LOAD, max_batch
    t, M = _table(), max_batch()
    stream = [(c, p) for c, p in t if p["stream"]]

    def some(what, pred, rows=stream):
        assert any(pred(c, p) for c, p in rows), what

    for q in ("int8", "f16"):
        E = LOAD[q]
        some(f"{q}: element loads because x alone is off alignment", lambda c, p: c[0] == q and c[2] % E == 0 and c[4] and not c[5] and not p["vec"])
        some(f"{q}: element loads because w alone is off alignment", lambda c, p: c[0] == q and c[2] % E == 0 and c[5] and not c[4] and not p["vec"])
        some(f"{q}: the pointer-only element loads with a K split", lambda c, p: c[0] == q and c[2] % E == 0 and (c[4] or c[5]) and p["S"] > 1)
        some(f"{q}: fewer slices than asked for", lambda c, p: c[0] == q and 1 < p["S"] < p["want"])
        some(f"{q}: a last slice of fewer than E elements",
             lambda c, p: c[0] == q and p["S"] > 1 and 0 < c[2] - (p["S"] - 1) * p["kslice"] < E)
        some(f"{q}: K below one load", lambda c, p: c[0] == q and c[2] < E)
        some(f"{q}: K == 1", lambda c, p: c[0] == q and c[2] == 1)
        some(f"{q}: ragged K on unaligned pointers with a K split", lambda c, p: c[0] == q and c[2] % E and c[4] and c[5] and p["S"] > 1)
        some(f"{q}: the workspace path at max + 1 rows", lambda c, p: c[0] == q and c[1] == M + 1, t)
        some(f"{q}: the workspace path at 17 rows", lambda c, p: c[0] == q and c[1] == 17, t)
        some(f"{q}: the workspace path on unaligned pointers", lambda c, p: c[0] == q and not p["stream"] and c[4] and c[5], t)
    for N in (1, 2, 3, 5, 15, 16, 17, 63, 65):
        some(f"N = {N}", lambda c, p: c[3] == N)
    some("N = 1 with a K split", lambda c, p: c[3] == 1 and p["S"] > 1)
    some("N >= 16 384: several K steps, no split asked for", lambda c, p: c[3] >= 16384 and p["want"] == 1 and p["S"] == 1 and p["steps"] > 1)
    some("N >= 16 384 with element loads", lambda c, p: c[3] >= 16384 and p["steps"] > 1 and not p["vec"])
    some("a ragged last workgroup behind full ones", lambda c, p: p["blocks_n"] > 1 and c[3] % 16 not in (0, 13, 14, 15))
    assert not any(p["stream"] for c, p in t if c[1] > M) and all(p["stream"] for c, p in t if c[1] <= M)
