"""bench.py's plain run and --dump-outputs: a plain line times exactly --steps steps and carries none of the records that take
runs of their own (those are --full's); the dumped arrays are what the timed path left behind, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT


def test_dump_helper_keeps_the_budget_and_samples_the_same_rows(tmp_path):
    import bench
    big = np.arange(200_000 * 64, dtype=np.float64).reshape(200_000, 64)           # 98 MB: above any share of the budget
    small = np.linspace(0.0, 1.0, 1000).astype(np.float32)
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), {"U": big, "p": small, "none": np.zeros(0)})
        assert rec["p"] == [[1000], None] and rec["none"] == [[0], None]
        assert rec["U"][1] is not None and rec["U"][0] == [rec["U"][1], 64]
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 * 2 ** 20
    ua, ub = np.load(str(tmp_path / "a" / "U.npy")), np.load(str(tmp_path / "b" / "U.npy"))
    assert ua.dtype == np.float64 and np.array_equal(ua, ub)                           # a fixed, seeded sample
    rows = ua[:, 0] / 64
    assert np.all(np.diff(rows) > 0) and np.array_equal(ua, big[rows.astype(np.int64)])  # whole rows, ascending
    p = np.load(str(tmp_path / "a" / "p.npy"))
    assert p.dtype == np.float64 and np.array_equal(p, small.astype(np.float64))


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith('{"metric"')]
    return json.loads(lines[-1]) if lines else None


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs(tmp_path):
    runs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                            "--dump-outputs", str(tmp_path / d)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        j = _line(r.stdout)
        assert r.returncode == 0 and j is not None and j["value"], (r.stdout[-800:], r.stderr[-3000:])
        runs.append(j)
    for j in runs:
        assert j["steps"] == 7 and j["repeats"] == 1 and j["prewarm_extra_steps"] == 256 and j["full"] is False
        assert j["ms_per_step"] > 0 and j["unit"] == "samples/s" and j["dtype"] == "f64" and j["higher_is_better"] is True
        assert not {"strong_10Mx1M", "bpmf_exe", "configs", "cpu_baseline"} & set(j)
        assert j["parity"]["value"] is None and "--full" in j["parity"]["reason"]
    a, b = tmp_path / "a", tmp_path / "b"
    names = sorted(os.listdir(str(a)))
    assert names == sorted(os.listdir(str(b))) == ["U.npy", "V.npy", "rmse.npy", "test_pred_avg.npy"]
    shapes = {"U.npy": (6040, 32), "V.npy": (3706, 32)}
    for n in names:
        x, y = np.load(str(a / n)), np.load(str(b / n))
        assert x.dtype == np.float64 and x.shape == y.shape and np.isfinite(x).all(), n
        if n in shapes:
            assert x.shape == shapes[n] and np.abs(x).max() > 0, n
        assert np.allclose(x, y, rtol=1e-9, atol=1e-12), (n, float(np.abs(x - y).max()))
    assert 0.1 < np.load(str(a / "rmse.npy"))[0] < 10.0
