"""The inclusion proof ABI (include/fd_bmtree_gpu.h): the descriptor's layout
against the numpy dtype, the header as C and as C++, the exported symbols,
calls refused before anything touches a device, and no result without one."""
import os
import subprocess

import numpy as np
import pytest

import bmtree_grid as bg
import bmtree_proof_grid as pg
import firedancer_amd as fa
from conftest import P, ROOT

SYMBOLS = ["fd_bmtree_proofs_batch", "fd_bmtree_gpu_proofs_packed", "fd_bmtree_gpu_proofs_dev", "fd_bmtree_from_proofs_batch",
           "fd_bmtree_gpu_from_proofs_packed", "fd_bmtree_gpu_from_proofs_dev"]


def _layout_asserts(kw):
    d = fa.BMTREE_PROOF_DTYPE
    lines = ['#include <stddef.h>', '#include "fd_bmtree_gpu.h"',
             f'{kw}( sizeof(fd_bmtree_gpu_proof_t) == {d.itemsize}, "proof" );']
    lines += [f'{kw}( offsetof(fd_bmtree_gpu_proof_t, {n}) == {d.fields[n][1]}, "{n}" );' for n in d.names]
    lines += [f'{kw}( FD_BMTREE_GPU_PROOF_EXPECT == {fa.BMTREE_PROOF_EXPECT}U, "flag" );',
              f'{kw}( FD_BMTREE_ERR_PROOF == {fa.BMTREE_ERR_PROOF}, "code" );',
              "int (*p_hemit)( unsigned, unsigned, unsigned long, uint32_t const *, fd_bmtree_gpu_leaf_t const *, void const *,"
              " unsigned long, unsigned long, void *, int *, void *, unsigned long, int ) = fd_bmtree_proofs_batch;",
              "int (*p_emit)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, uint32_t const *, fd_bmtree_gpu_leaf_t const *,"
              " void const *, unsigned long, unsigned long, void *, int *, void *, unsigned long ) = fd_bmtree_gpu_proofs_packed;",
              "int (*p_emit_dev)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, uint32_t const *, unsigned long,"
              " fd_bmtree_gpu_leaf_t const *, void const *, unsigned long, unsigned long, void *, unsigned long, void *, unsigned long,"
              " int *, void *, void * ) = fd_bmtree_gpu_proofs_dev;",
              "int (*p_hwalk)( unsigned, unsigned, unsigned long, fd_bmtree_gpu_proof_t const *, void const *, unsigned long,"
              " unsigned long, void *, int *, int ) = fd_bmtree_from_proofs_batch;",
              "int (*p_walk)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, fd_bmtree_gpu_proof_t const *, void const *,"
              " unsigned long, unsigned long, void *, int * ) = fd_bmtree_gpu_from_proofs_packed;",
              "int (*p_walk_dev)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, fd_bmtree_gpu_proof_t const *, void const *,"
              " unsigned long, unsigned long, void *, unsigned long, int *, void * ) = fd_bmtree_gpu_from_proofs_dev;", ""]
    return "\n".join(lines)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text(_layout_asserts("_Static_assert"))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_header_compiles_as_cxx(tmp_path):
    src = tmp_path / "abi.cpp"
    src.write_text(_layout_asserts("static_assert"))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_symbols_exported_and_python_names():
    L = fa.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    for m in ("bmtree_proofs", "bmtree_proofs_dev", "bmtree_from_proofs", "bmtree_from_proofs_dev"):
        assert callable(getattr(fa.Engine, m))
    assert callable(fa.bmtree_proofs_batch) and callable(fa.bmtree_from_proofs_batch)
    assert fa.BMTREE_PROOF_DTYPE.itemsize == 32 and fa.BMTREE_ERR_PROOF == -1


def _emit_inputs():
    cnt, leaves, blob = bg.sig_batch([2, 3], 6)            # 5 leaves, leaf_max 8: L = 3
    return cnt, leaves, blob, np.full((2, 32), 0x55, np.uint8), np.full(2, 77, np.int32), np.full((5, 96), pg.FILL, np.uint8)


def test_bad_emit_calls_are_refused_without_a_device():
    L = fa.lib()
    cnt, leaves, blob, roots, codes, rows = _emit_inputs()

    def host(**k):
        return L.fd_bmtree_proofs_batch(k.get("w", 32), k.get("f", 0), 2, k.get("cnt", P(cnt)), k.get("lv", P(leaves)), P(blob),
                                        blob.nbytes, k.get("lm", 8), k.get("r", P(roots)), k.get("c", P(codes)),
                                        k.get("p", P(rows)), k.get("stride", 96), k.get("th", 2))

    def packed(**k):
        return L.fd_bmtree_gpu_proofs_packed(None, k.get("w", 32), k.get("f", 0), k.get("n", 2), k.get("cnt", P(cnt)),
                                             k.get("lv", P(leaves)), P(blob), k.get("bsz", blob.nbytes), k.get("lm", 8),
                                             k.get("r", P(roots)), k.get("c", P(codes)), k.get("p", P(rows)), k.get("stride", 96))
    for call in (host, packed):
        assert call(stride=92) == fa.ERR_ARG               # 32 * 3 = 96 is the least
        assert call(stride=98) == fa.ERR_ARG               # not a multiple of 4
        assert call(p=None) == fa.ERR_ARG
        assert call(p=rows.ctypes.data + 2) == fa.ERR_ARG  # base not 4-aligned
        assert call(cnt=None) == fa.ERR_ARG
        assert call(lv=None) == fa.ERR_ARG
        assert call(r=None) == fa.ERR_ARG
        assert call(c=None) == fa.ERR_ARG
        assert call(w=24) == fa.ERR_ARG
        assert call(f=2) == fa.ERR_ARG
        assert call(lm=0) == fa.ERR_ARG
    assert host(th=0) == fa.ERR_ARG
    other = rows.copy()
    assert host(w=20, stride=60, p=P(other)) == 0          # 20 * 3 at the narrower width
    assert packed(bsz=1 << 32) == fa.ERR_ARG
    assert packed(n=0, cnt=None, lv=None, r=None, c=None, p=None) == 0

    def dev(**k):
        return L.fd_bmtree_gpu_proofs_dev(None, k.get("w", 20), k.get("f", 0), 2, k.get("first", 64), k.get("nl", 5), 128, 256, 320,
                                          k.get("lm", 8), k.get("r", 512), 32, k.get("p", 4096), k.get("stride", 60), 1024,
                                          k.get("work", 2048), None)
    assert dev(stride=56) == fa.ERR_ARG
    assert dev(stride=62) == fa.ERR_ARG
    assert dev(p=None) == fa.ERR_ARG
    assert dev(p=4098) == fa.ERR_ARG
    assert dev(lm=2, stride=16) == fa.ERR_ARG              # leaf_max 2: one level of 20 bytes
    assert dev(nl=1 << 31) == fa.ERR_ARG
    assert dev(first=None) == fa.ERR_ARG
    assert dev(work=None) == fa.ERR_ARG
    assert dev(f=0x80000000) == fa.ERR_ARG
    assert dev(w=21) == fa.ERR_ARG
    assert (rows == pg.FILL).all()


def test_bad_from_proofs_calls_are_refused_without_a_device():
    L = fa.lib()
    desc, blob, _ = pg.tree_walk_batch(20, [3, 2], False, 8)
    n = len(desc)
    roots = np.full((n, 32), 0x55, np.uint8)
    codes = np.full(n, 77, np.int32)

    def host(**k):
        return L.fd_bmtree_from_proofs_batch(k.get("w", 20), k.get("f", 0), k.get("n", n), k.get("d", P(desc)), k.get("b", P(blob)),
                                             blob.nbytes, k.get("dm", 2), k.get("r", P(roots)), k.get("c", P(codes)), k.get("th", 2))

    def packed(**k):
        return L.fd_bmtree_gpu_from_proofs_packed(None, k.get("w", 20), k.get("f", 0), k.get("n", n), k.get("d", P(desc)),
                                                  k.get("b", P(blob)), k.get("bsz", blob.nbytes), k.get("dm", 2),
                                                  k.get("r", P(roots)), k.get("c", P(codes)))
    for call in (host, packed):
        assert call(dm=0) == fa.ERR_ARG
        assert call(dm=33) == fa.ERR_ARG
        assert call(d=None) == fa.ERR_ARG
        assert call(b=None) == fa.ERR_ARG
        assert call(r=None) == fa.ERR_ARG
        assert call(c=None) == fa.ERR_ARG
        assert call(w=24) == fa.ERR_ARG
        assert call(f=2) == fa.ERR_ARG
        assert call(n=1 << 31) == fa.ERR_ARG
        assert call(n=0, d=None, b=None, r=None, c=None) == 0
    assert host(th=257) == fa.ERR_ARG
    assert packed(bsz=1 << 32) == fa.ERR_ARG

    def dev(**k):
        return L.fd_bmtree_gpu_from_proofs_dev(None, k.get("w", 20), k.get("f", 0), n, k.get("d", 64), 4096, 8192, k.get("dm", 2),
                                               k.get("r", 512), k.get("stride", 32), k.get("c", 1024), None)
    assert dev(dm=0) == fa.ERR_ARG
    assert dev(dm=33) == fa.ERR_ARG
    assert dev(d=None) == fa.ERR_ARG
    assert dev(r=None) == fa.ERR_ARG
    assert dev(c=None) == fa.ERR_ARG
    assert dev(r=514) == fa.ERR_ARG
    assert dev(stride=28) == fa.ERR_ARG
    assert dev(stride=34) == fa.ERR_ARG
    assert dev(d=66) == fa.ERR_ARG
    assert (roots == 0x55).all() and (codes == 77).all()


def test_no_device_no_result():
    if fa.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    L = fa.lib()
    cnt, leaves, blob, roots, codes, rows = _emit_inputs()
    assert L.fd_bmtree_gpu_proofs_packed(None, 32, 0, 2, P(cnt), P(leaves), P(blob), blob.nbytes, 8, P(roots), P(codes), P(rows),
                                         96) == fa.ERR_GPU
    assert (roots == 0x55).all() and (codes == 77).all() and (rows == pg.FILL).all()      # no host fallback
    assert L.fd_bmtree_gpu_proofs_dev(None, 20, 0, 2, 64, 5, 128, 256, 320, 8, 512, 32, 4096, 60, 1024, 2048, None) == fa.ERR_GPU
    desc, blob, _ = pg.tree_walk_batch(20, [3, 2], False, 8)
    roots = np.full((len(desc), 32), 0x55, np.uint8)
    codes = np.full(len(desc), 77, np.int32)
    assert L.fd_bmtree_gpu_from_proofs_packed(None, 20, 0, len(desc), P(desc), P(blob), blob.nbytes, 2, P(roots), P(codes)) == fa.ERR_GPU
    assert (roots == 0x55).all() and (codes == 77).all()
    assert L.fd_bmtree_gpu_from_proofs_dev(None, 20, 0, len(desc), 64, 4096, 8192, 2, 512, 32, 1024, None) == fa.ERR_GPU
