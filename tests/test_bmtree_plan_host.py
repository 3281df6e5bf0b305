"""The Merkle device call's plan arithmetic on the CPU
(firedancer_amd/csrc/fd_bmtree_gpu_private.h: fd_bmtree_plan_make,
fd_bmtree_plan_layout, fd_bmtree_layer_bound, fd_bmtree_ceil_log2).  A device
call launches its merge lanes and sizes its node buffers from the shapes
alone; a lane count or a capacity one too small gives a wrong root with code
0, not an error.  tests/bmtree_plan_harness.cpp, a stand-alone program under
UndefinedBehaviorSanitizer, holds the functions themselves to the exact layer
counts of every multiset of tree sizes with N <= 40, and checks that nothing
wraps at T = N = 0x7fffffff.  Nothing is preloaded and nothing is loaded into
Python."""
import os
import re
import subprocess

import bmtree_grid as bg
from conftest import ROOT


def _partitions(n_max):
    """p[n]: the multisets of positive sizes that sum to n"""
    p = [1] + [0] * n_max
    for part in range(1, n_max + 1):
        for n in range(part, n_max + 1):
            p[n] += p[n - part]
    return p


def test_plan_lanes_capacities_and_layout(tmp_path):
    exe = tmp_path / "bmtree_plan_harness"
    src = os.path.join(ROOT, "tests", "bmtree_plan_harness.cpp")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    san = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", *san, *inc, src, "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
    m = re.fullmatch(r"multisets (\d+) plans (\d+) layers (\d+) tight (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) big ok\n", r.stdout)
    assert m, r.stdout
    multisets, plans, layers, *tight = (int(x) for x in m.groups())
    p = _partitions(40)
    assert multisets == sum(p) == 215308
    # leaf_max in {1, 2, 3, N-1, N, 2^30} without repeats and without 0; 0 and 3 empty trees, T = 0 left out
    want = 0
    for N in range(41):
        lms = {lm for lm in (1, 2, 3, N - 1, N, 1 << 30) if lm >= 1}
        want += p[N] * len(lms) * (2 if N else 1)
    assert plans == want
    assert layers > plans
    # the bound has no slack: some shape meets it in every layer 1..6 (the issue's shapes are among them)
    assert all(t > 0 for t in tight), tight
    for shape, l in bg.TIGHT_LAYER.items():
        assert sum(shape) <= 40
        assert bg.layer_counts(shape, 1 << 30)[l - 1] == bg.layer_bound(len(shape), sum(shape), l)
