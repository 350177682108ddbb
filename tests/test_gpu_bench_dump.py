"""bench.py --dump-outputs end to end: the files are written, and two runs with the same arguments write the same arrays up to
rounding (the dumped step starts from the seeded initial state; fp32 atomic reductions still add in varying order).  `pytest -m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench_dump(out):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--bs", "8", "--steps", "2", "--warmup", "1", "--no-extras",
           "--no-cpu-baseline", "--no-parity", "--no-fp32-mode", "--no-vq-microbench", "--no-ae-only", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["codebook.npy", "losses.npy", "state_sample.npy"]
    return {n: np.load(os.path.join(out, n + ".npy")) for n in ("losses", "codebook", "state_sample")}


def test_bench_dump_outputs_repeat(dev, tmp_path):
    a, b = _bench_dump(tmp_path / "a"), _bench_dump(tmp_path / "b")
    assert a["losses"].shape == (2,) and a["codebook"].shape == (1024, 256)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all()
        scale = float(np.abs(a[k]).max())
        assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= 1e-5 * scale, k
