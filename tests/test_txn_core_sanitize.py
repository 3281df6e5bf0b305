"""The parser core as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/txn_core_harness.cpp with its own main
(-DTXN_HARNESS_MAIN) runs the test_mutate sweep of the three fixtures
through every mode of the core (no buffer, a buffer of exactly the
footprint, one byte less, the trusted single walk), each payload copied to
the end of a heap block of exactly its size, so a read one byte past the
payload is caught.  The grammar grid (tests/txn_grid.py) goes through the
same modes from a file of length-prefixed payloads (--grid).  An executable
of its own: nothing is preloaded and nothing is loaded into Python."""
import os
import subprocess

import txn_grid as tg
from conftest import GOLDEN
from test_txn_core_host import build_harness


def test_txn_core_under_asan_ubsan(tmp_path):
    exe = tmp_path / "txn_san"
    build_harness(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTXN_HARNESS_MAIN"))
    fx = [os.path.join(GOLDEN, f"transaction{i}.bin") for i in (1, 2, 3)]
    g = tg.grid()
    tg.write_file(g, tmp_path / "grid.bin")
    r = subprocess.run([str(exe), *fx, "--grid", str(tmp_path / "grid.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("payloads ok"), r.stdout + r.stderr
    assert f"{len(g.cases)} grid payloads ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
