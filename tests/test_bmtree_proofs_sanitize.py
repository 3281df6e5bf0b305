"""The inclusion proof host routines as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/bmtree_proof_harness.cpp
(its own main) linked with firedancer_amd/csrc/fd_bmtree_host.c, both
compiled with the sanitizers.  It runs the emit and the from-proofs cases of
tests/test_bmtree_proofs_host.py from files written here from the model, among
them a proof that ends on the blob's last byte.  An executable of its own:
nothing is preloaded and nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

import bmtree_grid as bg
import bmtree_proof_grid as pg
import firedancer_amd as fa
from conftest import ROOT

SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
NODES = fa.BMTREE_LEAVES_ARE_NODES


def _write_emit(path, W, nodes, cnt, leaves, blob, leaf_max):
    stride = pg.stride_of(W, cnt, leaf_max)
    roots, codes, rows = pg.emit_model(W, cnt, leaves, blob, leaf_max, nodes, stride)
    with open(path, "wb") as f:
        f.write(struct.pack("<8Q", 0, W, NODES if nodes else 0, len(cnt), len(leaves), len(blob), leaf_max, stride))
        f.write(np.ascontiguousarray(cnt, np.uint32).tobytes())
        f.write(np.ascontiguousarray(leaves, fa.BMTREE_LEAF_DTYPE).tobytes())
        f.write(np.ascontiguousarray(blob, np.uint8).tobytes())
        f.write(roots.tobytes())
        f.write(codes.tobytes())
        f.write(rows.tobytes())
    return len(cnt)


def _write_walk(path, W, nodes):
    desc, blob, depth_max, tags = pg.walk_cases(W, nodes)
    last = desc[[t for t, _ in tags].index("last")]
    assert int(last["proof_off"]) + int(last["depth"]) * W == len(blob)      # the proof that ends the blob
    roots, codes = pg.walk_model(W, desc, blob, depth_max, nodes)
    assert codes[[t for t, _ in tags].index("last")] == 0
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", 1, W, NODES if nodes else 0, len(desc), len(blob), depth_max))
        f.write(desc.tobytes())
        f.write(blob.tobytes())
        f.write(roots.tobytes())
        f.write(codes.tobytes())
    return len(desc)


def test_bmtree_proofs_host_under_asan_ubsan(tmp_path):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    obj, exe = tmp_path / "fd_bmtree_host.o", tmp_path / "bmtree_proof_san"
    subprocess.run(["gcc", *SAN, "-Wall", *inc, "-c", os.path.join(ROOT, "firedancer_amd", "csrc", "fd_bmtree_host.c"), "-o", str(obj)],
                   check=True, capture_output=True)
    subprocess.run(["g++", *SAN, "-std=c++17", "-Wall", *inc, os.path.join(ROOT, "tests", "bmtree_proof_harness.cpp"), str(obj),
                    "-o", str(exe), "-lpthread"], check=True, capture_output=True)
    files, total = [], 0
    for W in (20, 32):
        for nodes in (False, True):
            cnt, leaves, blob, leaf_max = pg.emit_grid(W, nodes)
            p = tmp_path / f"emit_{W}_{int(nodes)}.bin"
            total += _write_emit(p, W, nodes, cnt, leaves, blob, leaf_max)
            files.append(str(p))
            cnt, leaves, blob, leaf_max, _ = bg.refusal_batch(W, nodes)
            p = tmp_path / f"emit_refuse_{W}_{int(nodes)}.bin"
            total += _write_emit(p, W, nodes, cnt, leaves, blob, leaf_max)
            files.append(str(p))
            p = tmp_path / f"walk_{W}_{int(nodes)}.bin"
            total += _write_walk(p, W, nodes)
            files.append(str(p))
    r = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{total} items ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
