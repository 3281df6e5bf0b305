"""The Proof-of-History host routines as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/poh_core_harness.cpp
(its own main) linked with firedancer_amd/csrc/fd_poh_host.c, both compiled
with the sanitizers.  It runs the case grid (entries the header refuses and
one-bit-wrong expects included) and mainnet block 1 against results written
here from hashlib.  An executable of its own: nothing is preloaded and
nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import firedancer_amd as fa
import poh_grid as pg
from conftest import ROOT

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def _write(path, ent, n_max, codes, states):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(ent), n_max))
        f.write(ent.tobytes())
        f.write(np.ascontiguousarray(codes, np.int32).tobytes())
        f.write(np.ascontiguousarray(states, np.uint8).tobytes())


def test_poh_host_under_asan_ubsan(tmp_path):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    obj, exe = tmp_path / "fd_poh_host.o", tmp_path / "poh_san"
    subprocess.run(["gcc", *SAN, "-Wall", *inc, "-c", os.path.join(ROOT, "firedancer_amd", "csrc", "fd_poh_host.c"), "-o", str(obj)],
                   check=True, capture_output=True)
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", *inc, os.path.join(ROOT, "tests", "poh_core_harness.cpp"), str(obj),
                    "-o", str(exe), "-lpthread"], check=True, capture_output=True)
    files, total = [], 0
    for C in (1, 4, 64):
        for count in (1, 63, 64, 65, 130):
            ent, codes, states = pg.grid(C, count)
            # entries the header refuses: unknown flag, nonzero _pad, n > n_max
            for k, i in enumerate(range(2, count, 11)):
                if k % 3 == 0:
                    ent[i]["flags"] |= 4
                elif k % 3 == 1:
                    ent[i]["_pad"] = 9
                else:
                    ent[i]["n"] = 2 * C + 2
                codes[i], states[i] = fa.ERR_ARG, 0
            p = tmp_path / f"grid_{C}_{count}.bin"
            _write(p, ent, 2 * C + 1, codes, states)
            files.append(str(p))
            total += count
    ent, _ = pg.block1_entries()
    _write(tmp_path / "block1.bin", ent, 1 << 20, np.zeros(len(ent), np.int32), ent["expect"])
    files.append(str(tmp_path / "block1.bin"))
    total += len(ent)
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{total} entries ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
