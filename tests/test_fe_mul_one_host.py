"""fd_fe_mul_one (firedancer_amd/csrc/fd_ed25519_gpu_fe.h): the by-one lanes
of the cached-form conversion [1, 1, 1, 2d] without their multiplies.  A
stand-alone host program (tests/fe_mul_one_host.cpp) holds it limb for limb
to fd_fe_mul( f, one ) -- which tests/test_fe_host.py holds to the
reference's AVX field path -- on more than 10^5 seeded inputs: carried
limbs, the unreduced sums the Ai precompute feeds in, limbs at 0, +-1,
+-2^25, +-2^26 and the int32 extremes, and arbitrary int32 limbs.  Runs on
the CPU."""
import os
import re
import subprocess

from conftest import ROOT


def test_fe_mul_one_equals_fe_mul_by_one(tmp_path):
    exe = tmp_path / "fe_mul_one_host"
    src = os.path.join(ROOT, "tests", "fe_mul_one_host.cpp")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", *inc, src, "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    classes = dict(re.findall(r"^(\w+)\s+(\d+) inputs, 0 mismatches$", r.stdout, re.M))
    assert set(classes) == {"carried", "unreduced", "edges", "int32", "total"}, r.stdout
    assert int(classes["total"]) >= 100000
