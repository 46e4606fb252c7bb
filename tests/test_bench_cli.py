"""bench.py's command line without a GPU: the options a plain and a --full run
take, and --dump-outputs' files (the counts a caller of the check receives)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_options_are_there():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in p.stdout


def test_zero_steps_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_dump_outputs_writes_the_counts_and_levels(tmp_path):
    res = dict(generated=6748471652, distinct=1885410558, left=0, depth=69, status="ok", hidden_var_collisions=7,
               levels=[[1, 1], [3, 3], [12, 9]], seconds=1.0, hash_capacity=1 << 32)
    bench.dump_outputs(str(tmp_path / "out"), res)
    counts, levels = np.load(tmp_path / "out" / "counts.npy"), np.load(tmp_path / "out" / "levels.npy")
    assert counts.dtype == np.float64 and levels.dtype == np.float64
    assert counts.tolist() == [6748471652, 1885410558, 0, 69, 0, 7]
    assert levels.tolist() == [[1, 1], [3, 3], [12, 9]]
    assert sorted(os.listdir(tmp_path / "out")) == ["counts.npy", "levels.npy"]
