"""The Merkle tree ABI (include/fd_bmtree_gpu.h and the entries calls of
include/fd_poh_gpu.h): layouts against the numpy dtypes, the header as C and
as C++, the exported symbols, calls refused before anything touches a
device, and no result without one."""
import os
import subprocess

import numpy as np
import pytest

import bmtree_grid as bg
import firedancer_amd as fa
from conftest import P, ROOT

SYMBOLS = [f"fd_bmtree{w}_{f}" for w in (20, 32)
           for f in ("hash_leaf", "commit_align", "commit_footprint", "commit_init", "commit_leaf_cnt", "commit_append", "commit_fini")]
SYMBOLS += ["fd_bmtree_roots_batch", "fd_bmtree_gpu_roots_packed", "fd_bmtree_gpu_roots_dev", "fd_bmtree_gpu_work_sz",
            "fd_bmtree_gpu_merge_passes", "fd_poh_gpu_verify_entries_packed", "fd_poh_gpu_verify_entries_dev",
            "fd_poh_gpu_entries_work_sz"]


def _layout_asserts(kw):
    al = "_Alignof" if kw == "_Static_assert" else "alignof"
    lines = ['#include <stddef.h>', '#include "fd_poh_gpu.h"',
             f'{kw}( sizeof(fd_bmtree_gpu_leaf_t) == {fa.BMTREE_LEAF_DTYPE.itemsize}, "leaf" );',
             f'{kw}( offsetof(fd_bmtree_gpu_leaf_t, off) == 0 && offsetof(fd_bmtree_gpu_leaf_t, sz) == 4, "leaf fields" );',
             f'{kw}( FD_BMTREE_GPU_LEAVES_ARE_NODES == {fa.BMTREE_LEAVES_ARE_NODES}U, "flag" );',
             f'{kw}( FD_BMTREE_GPU_LEAF_SZ_MAX == {fa.BMTREE_LEAF_SZ_MAX}U, "leaf size" );']
    for w in (20, 32):
        lines += [f'{kw}( sizeof(fd_bmtree{w}_node_t) == 32 && {al}(fd_bmtree{w}_node_t) == 32, "node{w}" );',
                  f'{kw}( sizeof(fd_bmtree{w}_commit_t) == 2048 && {al}(fd_bmtree{w}_commit_t) == 32, "commit{w}" );',
                  f'{kw}( FD_BMTREE{w}_COMMIT_FOOTPRINT == 2048UL && FD_BMTREE{w}_COMMIT_ALIGN == 32UL && FD_BMTREE{w}_HASH_SZ == {w}UL, "c{w}" );',
                  f"fd_bmtree{w}_node_t * (*p_leaf{w})( fd_bmtree{w}_node_t *, void const *, unsigned long ) = fd_bmtree{w}_hash_leaf;",
                  f"fd_bmtree{w}_commit_t * (*p_app{w})( fd_bmtree{w}_commit_t *, fd_bmtree{w}_node_t const *, unsigned long )"
                  f" = fd_bmtree{w}_commit_append;",
                  f"uint8_t * (*p_fini{w})( fd_bmtree{w}_commit_t * ) = fd_bmtree{w}_commit_fini;"]
    lines += ["int (*p_packed)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, uint32_t const *, fd_bmtree_gpu_leaf_t const *,"
              " void const *, unsigned long, unsigned long, void *, int * ) = fd_bmtree_gpu_roots_packed;",
              "int (*p_dev)( fd_ed25519_gpu_t *, unsigned, unsigned, unsigned long, uint32_t const *, unsigned long,"
              " fd_bmtree_gpu_leaf_t const *, void const *, unsigned long, unsigned long, void *, unsigned long, int *, void *, void * )"
              " = fd_bmtree_gpu_roots_dev;",
              "int (*p_ent)( fd_ed25519_gpu_t *, unsigned long, fd_poh_gpu_entry_t const *, unsigned long, int *, void *,"
              " uint32_t const *, fd_bmtree_gpu_leaf_t const *, void const *, unsigned long, unsigned long )"
              " = fd_poh_gpu_verify_entries_packed;", ""]
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
    for m in ("bmtree_roots", "bmtree_roots_dev", "poh_verify_entries", "poh_verify_entries_dev"):
        assert callable(getattr(fa.Engine, m))
    for f in (fa.bmtree_hash_leaf, fa.bmtree_roots_batch, fa.bmtree_work_sz, fa.bmtree_merge_passes, fa.poh_entries_work_sz,
              fa.BmtreeCommit):
        assert callable(f)
    assert fa.BMTREE_LEAF_DTYPE.itemsize == 8


@pytest.mark.parametrize("shape", [(0, 0), (1, 1), (5, 0), (3, 1000), (1000, 37)])
def test_work_sz(shape):
    T, N = shape
    w = fa.bmtree_work_sz(T, N)
    assert w % 16 == 0
    assert w >= 32 * N + 32 * (2 * N // 3) + 4 * T          # both node buffers and a word per tree
    assert fa.poh_entries_work_sz(T, N) >= w + 4 * T
    assert fa.bmtree_work_sz(1 << 31, 1) == 0 and fa.bmtree_work_sz(1, 1 << 31) == 0


def test_bad_calls_are_refused_without_a_device():
    L = fa.lib()
    cnt, leaves, blob = bg.sig_batch([2, 3], 6)
    roots = np.full((2, 32), 0x55, np.uint8)
    codes = np.full(2, 77, np.int32)

    def packed(**k):
        return L.fd_bmtree_gpu_roots_packed(None, k.get("w", 32), k.get("f", 0), k.get("n", 2), k.get("cnt", P(cnt)),
                                            k.get("lv", P(leaves)), P(blob), k.get("bsz", blob.nbytes), k.get("lm", 8),
                                            k.get("r", P(roots)), k.get("c", P(codes)))
    assert packed(w=24) == fa.ERR_ARG
    assert packed(w=0) == fa.ERR_ARG
    assert packed(f=2) == fa.ERR_ARG
    assert packed(f=0x80000000) == fa.ERR_ARG
    assert packed(cnt=None) == fa.ERR_ARG
    assert packed(lv=None) == fa.ERR_ARG
    assert packed(r=None) == fa.ERR_ARG
    assert packed(c=None) == fa.ERR_ARG
    assert packed(lm=0) == fa.ERR_ARG
    assert packed(bsz=1 << 32) == fa.ERR_ARG
    assert packed(n=1 << 31) == fa.ERR_ARG
    assert packed(n=0, cnt=None, lv=None, r=None, c=None) == 0

    def dev(**k):
        return L.fd_bmtree_gpu_roots_dev(None, k.get("w", 20), k.get("f", 0), 2, k.get("first", 64), k.get("nl", 5), 128, 256, 320,
                                         k.get("lm", 8), k.get("r", 512), k.get("stride", 32), 1024, k.get("work", 2048), None)
    assert dev(w=21) == fa.ERR_ARG
    assert dev(f=0x80000000) == fa.ERR_ARG                    # the private flag is not the public call's
    assert dev(first=None) == fa.ERR_ARG
    assert dev(r=None) == fa.ERR_ARG
    assert dev(work=None) == fa.ERR_ARG
    assert dev(work=2056) == fa.ERR_ARG                       # d_work not 16-aligned
    assert dev(r=514) == fa.ERR_ARG                           # d_roots not 4-aligned
    assert dev(stride=28) == fa.ERR_ARG
    assert dev(stride=34) == fa.ERR_ARG
    assert dev(lm=0) == fa.ERR_ARG
    assert dev(nl=1 << 31) == fa.ERR_ARG

    ent = np.zeros(2, fa.POH_ENTRY_DTYPE)
    out = np.full(2, 77, np.int32)

    def entries(**k):
        return L.fd_poh_gpu_verify_entries_packed(None, 2, k.get("ent", P(ent)), 1, P(out), None, k.get("cnt", P(cnt)),
                                                  k.get("lv", P(leaves)), P(blob), k.get("bsz", blob.nbytes), k.get("lm", 8))
    assert entries(ent=None) == fa.ERR_ARG
    assert entries(cnt=None) == fa.ERR_ARG
    assert entries(lv=None) == fa.ERR_ARG
    assert entries(lm=0) == fa.ERR_ARG
    assert entries(bsz=1 << 32) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_entries_dev(None, 2, 112, 1, 1024, None, 2048, None, 5, 128, 256, 320, 8, 4096, None) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_entries_dev(None, 2, 112, 1, 1024, None, 2048, 64, 5, 128, 256, 320, 8, 4100, None) == fa.ERR_ARG
    assert (roots == 0x55).all() and (codes == 77).all() and (out == 77).all()


def test_no_device_no_result():
    if fa.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    cnt, leaves, blob = bg.sig_batch([2, 3], 6)
    roots = np.full((2, 32), 0x55, np.uint8)
    codes = np.full(2, 77, np.int32)
    L = fa.lib()
    assert L.fd_bmtree_gpu_roots_packed(None, 32, 0, 2, P(cnt), P(leaves), P(blob), blob.nbytes, 8, P(roots), P(codes)) == fa.ERR_GPU
    assert (roots == 0x55).all() and (codes == 77).all()      # no host fallback
    ent = np.zeros(2, fa.POH_ENTRY_DTYPE)
    out = np.full(2, 77, np.int32)
    assert L.fd_poh_gpu_verify_entries_packed(None, 2, P(ent), 1, P(out), None, P(cnt), P(leaves), P(blob), blob.nbytes, 8) == fa.ERR_GPU
    assert (out == 77).all()
    with pytest.raises(fa.EngineError):
        fa.Engine(0, 16, 4096)
