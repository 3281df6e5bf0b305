"""The Proof-of-History ABI (include/fd_poh_gpu.h): the entry's layout
against the numpy dtype, the codes, the header as C and as C++, the
exported symbols, and calls refused before anything touches a device."""
import os
import subprocess

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P, ROOT

SYMBOLS = ["fd_poh_append", "fd_poh_mixin", "fd_poh_verify_batch", "fd_poh_gpu_verify_packed", "fd_poh_gpu_verify_dev",
           "fd_poh_gpu_work_sz", "fd_poh_gpu_chain", "fd_poh_gpu_debug_set_chunk", "fd_poh_gpu_chunk"]

FIELDS = ("start", "mixin", "expect", "n", "flags", "_pad")


def _layout_asserts(kw):
    dt = fa.POH_ENTRY_DTYPE
    lines = ['#include <stddef.h>', '#include "fd_poh_gpu.h"',
             f'{kw}( sizeof(fd_poh_gpu_entry_t) == {dt.itemsize}, "size" );',
             f'{kw}( _Alignof(fd_poh_gpu_entry_t) == 8, "alignment" );' if kw == "_Static_assert"
             else f'{kw}( alignof(fd_poh_gpu_entry_t) == 8, "alignment" );']
    for f in FIELDS:
        lines.append(f'{kw}( offsetof(fd_poh_gpu_entry_t, {f}) == {dt.fields[f][1]}, "{f}" );')
    lines += [f'{kw}( FD_POH_GPU_MIXIN == {fa.POH_MIXIN}U, "flag" );',
              f'{kw}( FD_POH_ERR_HASH == {fa.POH_ERR_HASH}, "code" );',
              f'{kw}( FD_ED25519_ERR_ARG == {fa.ERR_ARG} && FD_ED25519_ERR_GPU == {fa.ERR_GPU}, "codes" );',
              f'{kw}( FD_POH_GPU_CHUNK_DEFAULT == {fa.POH_CHUNK_DEFAULT}UL, "chunk" );',
              f'{kw}( sizeof(fd_poh_state_t) == 32, "state" );',
              "fd_poh_state_t * (*p_append)( fd_poh_state_t *, unsigned long ) = fd_poh_append;",
              "fd_poh_state_t * (*p_mixin)( fd_poh_state_t *, uint8_t const * ) = fd_poh_mixin;",
              "int (*p_batch)( unsigned long, fd_poh_gpu_entry_t const *, unsigned long, int *, void *, int ) = fd_poh_verify_batch;",
              "int (*p_packed)( fd_ed25519_gpu_t *, unsigned long, fd_poh_gpu_entry_t const *, unsigned long, int *, void * )"
              " = fd_poh_gpu_verify_packed;",
              "int (*p_dev)( fd_ed25519_gpu_t *, unsigned long, fd_poh_gpu_entry_t const *, unsigned long, int *, void *, void *,"
              " void * ) = fd_poh_gpu_verify_dev;", ""]
    return "\n".join(lines)


def test_dtype_layout():
    dt = fa.POH_ENTRY_DTYPE
    assert dt.itemsize == 112
    assert [dt.fields[f][1] for f in FIELDS] == [0, 32, 64, 96, 104, 108]
    assert fa.POH_ERR_HASH == -1 and fa.POH_MIXIN == 1


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


def test_symbols_exported():
    L = fa.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    for m in ("poh_verify", "poh_verify_dev"):
        assert callable(getattr(fa.Engine, m))
    for f in (fa.poh_append, fa.poh_mixin, fa.poh_verify_batch, fa.poh_chain):
        assert callable(f)
    assert fa.poh_work_sz(10) == 480 and fa.poh_work_sz(0) > 0


def test_bad_calls_are_refused_without_a_device():
    L = fa.lib()
    ent = np.zeros(2, fa.POH_ENTRY_DTYPE)
    out = np.full(2, 77, np.int32)
    assert L.fd_poh_gpu_verify_packed(None, 2, None, 1, P(out), None) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_packed(None, 2, P(ent), 1, None, None) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_packed(None, 1 << 31, P(ent), 1, P(out), None) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_packed(None, 0, None, 1, None, None) == 0
    assert L.fd_poh_gpu_verify_dev(None, 2, None, 1, P(out), None, P(out), None) == fa.ERR_ARG
    assert L.fd_poh_gpu_verify_dev(None, 2, P(ent), 1, P(out), None, 8, None) == fa.ERR_ARG      # d_work not 16-aligned
    assert L.fd_poh_gpu_verify_dev(None, 0, None, 1, None, None, None, None) == 0
    assert L.fd_poh_gpu_debug_set_chunk(None, (1 << 24) + 1) == fa.ERR_ARG
    assert (out == 77).all()


@pytest.mark.parametrize("n", [0, 1, 5])
def test_work_sz(n):
    assert fa.poh_work_sz(n) == 48 * max(n, 1)
