"""The transaction ABI (include/fd_ed25519_gpu_txn.h): the header is C, the
two structs have the documented layout, the symbols are exported, the new
code has its value and string, malformed calls are refused before anything
touches a device, and the verify kernels' build id is the one it was before
the transaction kernels were added (they live outside the Makefile's KSRC)."""
import ctypes
import os
import subprocess

import numpy as np

import firedancer_amd as fa
from conftest import P, ROOT
from firedancer_amd import txn

SYMBOLS = ["fd_ed25519_gpu_txns_reserve", "fd_ed25519_gpu_verify_txns_dev", "fd_ed25519_gpu_verify_txns_packed",
           "fd_ed25519_gpu_debug_txn_descs", "fd_ed25519_gpu_verify_txns_dev_timed"]

# fd_ed25519_gpu_kernels_id() of the commit before this header existed
KERNELS_ID_BEFORE = "f8cd592cbcd9b28d"

LAYOUT = """
#include <stddef.h>
#include "fd_ed25519_gpu_txn.h"
#define AT(t, f, o) _Static_assert( offsetof(t, f) == (o), #f )
_Static_assert( sizeof(fd_ed25519_gpu_txn_t) == 8, "entry" );
AT( fd_ed25519_gpu_txn_t, off, 0 ); AT( fd_ed25519_gpu_txn_t, sz, 4 );
_Static_assert( sizeof(fd_ed25519_gpu_txn_result_t) == 24, "result" );
AT( fd_ed25519_gpu_txn_result_t, status, 0 );     AT( fd_ed25519_gpu_txn_result_t, sig_base, 4 );
AT( fd_ed25519_gpu_txn_result_t, tag, 8 );        AT( fd_ed25519_gpu_txn_result_t, footprint, 16 );
AT( fd_ed25519_gpu_txn_result_t, reject_line, 18 ); AT( fd_ed25519_gpu_txn_result_t, sig_cnt, 20 );
AT( fd_ed25519_gpu_txn_result_t, version, 21 );   AT( fd_ed25519_gpu_txn_result_t, _pad, 22 );
_Static_assert( FD_ED25519_ERR_TXN == -18 && FD_ED25519_ERR_TXN == FD_ED25519_ERR_GPU - 1, "the next free code" );
int (*p_dev)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *, unsigned long,
              fd_ed25519_gpu_txn_result_t *, int *, void *, unsigned long, void * ) = fd_ed25519_gpu_verify_txns_dev;
int (*p_pk)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *,
             fd_ed25519_gpu_txn_result_t *, int *, void *, unsigned long ) = fd_ed25519_gpu_verify_txns_packed;
int (*p_rs)( fd_ed25519_gpu_t *, unsigned long ) = fd_ed25519_gpu_txns_reserve;
int (*p_dbg)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *, unsigned long,
              fd_ed25519_gpu_desc_t *, unsigned long *, fd_ed25519_gpu_txn_result_t * ) = fd_ed25519_gpu_debug_txn_descs;
"""


def test_header_is_c_with_the_documented_layout(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_python_mirrors_the_structs():
    assert fa.TXN_DTYPE.itemsize == 8 and [fa.TXN_DTYPE.fields[f][1] for f in ("off", "sz")] == [0, 4]
    r = fa.TXN_RESULT_DTYPE
    assert r.itemsize == 24
    assert [r.fields[f][1] for f in ("status", "sig_base", "tag", "footprint", "reject_line", "sig_cnt", "version", "_pad")] == [
        0, 4, 8, 16, 18, 20, 21, 22]
    blob, t = txn.pack([b"abc", b"", b"de"], gap=3, first=1)
    assert t.dtype == fa.TXN_DTYPE and t.tolist() == [(1, 3), (7, 0), (10, 2)]
    assert bytes(blob[:12]) == b"\0abc\0\0\0\0\0\0de" and len(blob) == 15 + 64


def test_symbols_exported():
    L = fa.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    for m in ("verify_txns", "verify_txns_dev", "txns_reserve", "debug_txn_descs"):
        assert callable(getattr(fa.Engine, m))


def test_err_txn_value_and_string():
    assert fa.ERR_TXN == -18 == fa.ERR_GPU - 1
    assert fa.strerror(fa.ERR_TXN) == "malformed transaction"
    # the reference's four and the engine's two are as they were
    assert [fa.strerror(c) for c in (0, -1, -2, -3, -16, -17, -19)] == [
        "success", "bad signature", "bad public key", "bad message", "bad argument", "gpu failure", "unknown"]


def test_null_engine_is_err_arg():
    L = fa.lib()
    buf = np.zeros(256, np.uint8)
    t = np.zeros(1, fa.TXN_DTYPE)
    res = np.zeros(1, fa.TXN_RESULT_DTYPE)
    n = ctypes.c_ulong(7)
    assert L.fd_ed25519_gpu_txns_reserve(None, 16) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_verify_txns_packed(None, 1, P(buf), 128, P(t), P(res), None, None, 0) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_verify_txns_dev(None, 1, P(buf), 128, P(t), 1, P(res), None, None, 0, None) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_debug_txn_descs(None, 1, P(buf), 128, P(t), 1, P(buf), ctypes.byref(n), None) == fa.ERR_ARG
    assert not res.view(np.uint8).any() and n.value == 7


def test_verify_kernels_build_id_unchanged():
    """the transaction kernels and their headers are outside KSRC: adding them left the id
    alone (a change that edits the verify kernels themselves moves it, and this constant)"""
    assert fa.kernels_id() == KERNELS_ID_BEFORE
    mk = open(os.path.join(ROOT, "firedancer_amd", "Makefile")).read()
    ksrc = mk[mk.index("KSRC :="):mk.index("KID  :=")]
    assert "txn" not in ksrc
