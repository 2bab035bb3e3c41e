"""Writes tests/golden/batchnorm_bits.npz: the bit patterns that th_batchnorm2d_fwd / th_batchnorm2d_bwd give on an MI355X for one case
per kernel form -- what tests/test_gpu_batchnorm.py::test_bits_match_the_recorded_parent compares against.  The inputs come from integer
formulas and the calls are the test's own (bits_record), so the fixture depends on the kernels' order of operations and on nothing else.
Run it on the GPU, with the library built, only when a change of the summation order is intended:

    python tests/golden/make_golden_batchnorm_bits.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from taper_amd import hip  # noqa: E402
from tests import test_gpu_batchnorm as G  # noqa: E402

if __name__ == "__main__":
    ctx = hip.Ctx(0)
    out = {}
    for shape, split in G.BIT_CASES.items():
        assert G._lib().th_batchnorm2d_split(shape[0], shape[1], shape[2] * shape[3]) == split, shape
        out["x".join(map(str, shape))] = np.concatenate(list(G.bits_record(ctx, shape).values()))
    ctx.close()
    np.savez(HERE / "batchnorm_bits.npz", **out)
    print(f"{len(out)} cases, {sum(a.nbytes for a in out.values())} bytes")
