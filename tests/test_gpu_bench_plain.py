"""GPU: bench.py's plain run (no --full) at a reduced size: the line counts the steps it was asked for, and --dump-outputs
writes the last timed step's results, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, steps):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--utts", "200", "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(out), "--blocks-out", str(tmp_path / (name + ".json"))],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, out


def test_plain_run_counts_its_steps_and_dumps_its_outputs(built_lib, tmp_path):
    a, da = _run(tmp_path, "a", 3)
    b, db = _run(tmp_path, "b", 2)
    for line, steps in ((a, 3), (b, 2)):
        assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert abs(line["value"] - 200 * 1000 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
        assert line["cpu_baseline"]["value"] is None and line["roofline"]["traffic"] is None          # --full only
    sums, arg = np.load(da / "sums.npy"), np.load(da / "argmax.npy")
    assert sums.shape == (200, 201) and sums.dtype == np.float64 and arg.shape == (200,) and arg.dtype == np.float64
    assert np.all(np.isfinite(sums)) and np.array_equal(arg, np.argmax(sums, axis=1))
    assert np.array_equal(sums, np.load(db / "sums.npy")) and np.array_equal(arg, np.load(db / "argmax.npy"))
