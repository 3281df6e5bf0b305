"""The Merkle tree host routines as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/bmtree_core_harness.cpp
(its own main) linked with firedancer_amd/csrc/fd_bmtree_host.c, both
compiled with the sanitizers.  It runs tree counts and leaf sizes around
every SHA-256 padding edge, node mode and every refusal against results
written here from the model.  An executable of its own: nothing is preloaded
and nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import bmtree_grid as bg
import firedancer_amd as fa
from conftest import ROOT

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def _write(path, W, flags, cnt, leaves, blob, leaf_max):
    roots, codes = bg.model(W, cnt, leaves, blob, leaf_max, bool(flags & fa.BMTREE_LEAVES_ARE_NODES))
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", W, flags, len(cnt), len(leaves), len(blob), leaf_max))
        f.write(np.ascontiguousarray(cnt, np.uint32).tobytes())
        f.write(np.ascontiguousarray(leaves, fa.BMTREE_LEAF_DTYPE).tobytes())
        f.write(np.ascontiguousarray(blob, np.uint8).tobytes())
        f.write(roots.tobytes())
        f.write(codes.tobytes())
    return len(cnt)


def test_bmtree_host_under_asan_ubsan(tmp_path):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    obj, exe = tmp_path / "fd_bmtree_host.o", tmp_path / "bmtree_san"
    subprocess.run(["gcc", *SAN, "-Wall", *inc, "-c", os.path.join(ROOT, "firedancer_amd", "csrc", "fd_bmtree_host.c"), "-o", str(obj)],
                   check=True, capture_output=True)
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", *inc, os.path.join(ROOT, "tests", "bmtree_core_harness.cpp"), str(obj),
                    "-o", str(exe), "-lpthread"], check=True, capture_output=True)
    rng = np.random.default_rng(77)
    files, total = [], 0
    for W in (20, 32):
        # tree sizes, 64-byte leaves
        cnt, leaves, blob = bg.sig_batch(list(range(1, 40)) + [63, 64, 65, 129], 70 + W)
        p = tmp_path / f"counts_{W}.bin"
        total += _write(p, W, 0, cnt, leaves, blob, 129)
        files.append(str(p))
        # leaf sizes around the padding edges, every start alignment, the last leaf ending the blob
        sizes = list(range(0, 131)) + [1203, 1228]
        trees = [[rng.bytes(s), rng.bytes(sizes[(i + 7) % len(sizes)]), rng.bytes(s)] for i, s in enumerate(sizes)]
        cnt, leaves, blob = bg.pack(trees, align_of=lambda k: k)
        p = tmp_path / f"sizes_{W}.bin"
        total += _write(p, W, 0, cnt, leaves, blob, 3)
        files.append(str(p))
        for nodes in (False, True):
            cnt, leaves, blob, leaf_max, _ = bg.refusal_batch(W, nodes)
            p = tmp_path / f"refuse_{W}_{int(nodes)}.bin"
            total += _write(p, W, fa.BMTREE_LEAVES_ARE_NODES if nodes else 0, cnt, leaves, blob, leaf_max)
            files.append(str(p))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{total} trees ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
