"""bench.py's command line on the GPU, at the smallest step that still takes
the throughput path's pooled DSM (64 batches of 4096 signatures =
FD_DSM_POOL_MIN_DEFAULT): a plain run carries the headline only and --dump-outputs writes
the codes of the timed steps; --full (here trimmed by --no-cpu --no-latency,
which imply it) adds the roofline (the reference check belongs to the CPU leg)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--step-batches", "64"]
FULL_ONLY = ("roofline", "latency", "c2_streamed", "cpu_baseline", "reference_check")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_timed_codes(tmp_path):
    import bench
    res = _bench("--dump-outputs", str(tmp_path))
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["codes_ok"] is True
    assert not [k for k in FULL_ONLY if k in res]
    n = res["config"]["sigs_per_step_per_gpu"]
    assert n == 64 * bench.BATCH_SIGS
    codes = np.load(tmp_path / "codes.npy")
    assert codes.dtype == np.float32 and codes.shape == (n,)
    assert not (codes == bench.CODE_UNWRITTEN).any()        # every entry written by a timed step
    u, c = np.unique(codes.astype(np.int64), return_counts=True)
    assert {str(int(k)): int(v) for k, v in zip(u, c)} == res["codes"]     # and equal to the checked first step's


def test_trimmed_full_run_has_roofline_without_the_trimmed_legs():
    res = _bench("--no-cpu", "--no-latency")
    assert res["codes_ok"] is True
    assert set(res["roofline"]["per_kernel"]) >= {"fd_k_prep", "fd_k_decomp", "fd_k_dsm_pool"}
    assert "latency" not in res and "cpu_baseline" not in res and "c2_streamed" not in res
