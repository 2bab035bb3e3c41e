"""bench.py's plain run (`python bench.py --gpus 1 --steps K --warmup W`): the headline only, exactly K timed steps, and with
--dump-outputs DIR what the last of them computed, the same from run to run (seeded inputs, fixed-order sums: bit-identical)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir, steps=20, warmup=5):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {p.stem: np.load(p) for p in sorted(Path(out_dir).glob("*.npy"))}


def test_plain_run_times_k_steps_and_dumps_the_last_step_reproducibly(tmp_path):
    d, out = _bench(tmp_path / "a")
    assert d["metric"] == "MNIST samples/sec fwd+bwd+step" and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5
    assert d["config"]["workload"] == "mlp_784-128-10_b64" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(64 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    # what only --full measures is absent from a plain run
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["details"] is None
    assert not {"workloads", "data_parallel", "batch_sweep_us_epochs_frac", "sustained_ms_per_step"} & set(d)

    assert set(out) == {"loss", "ncorrect", "param0", "param1", "param2", "param3"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert sum(out[f"param{i}"].size for i in range(4)) == 101_770          # MLP 784-128-10: every weight and bias after the last Adam update
    assert out["loss"].shape == (1,) and 0.0 < out["loss"][0] < 10.0
    assert out["ncorrect"].shape == (1,) and 0 <= out["ncorrect"][0] <= 64 and out["ncorrect"][0] == int(out["ncorrect"][0])

    _, again = _bench(tmp_path / "b")
    for k in out:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
