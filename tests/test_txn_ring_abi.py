"""The ABI of transactions through the ring (include/fd_ed25519_gpu_txn.h:
fd_ed25519_gpu_txn_claims, _try_submit_txns, _submit_txns, _poll_txns): the
header is C, the symbols and their Python names exist, malformed calls are
refused before anything touches a device, and without a device nothing
pretends to work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P, ROOT

SYMBOLS = ["fd_ed25519_gpu_txn_claims", "fd_ed25519_gpu_try_submit_txns", "fd_ed25519_gpu_submit_txns", "fd_ed25519_gpu_poll_txns"]

PROTOS = """
#include "fd_ed25519_gpu_txn.h"
unsigned long (*p_cl)( void const *, unsigned long, fd_ed25519_gpu_txn_t const *, unsigned long, uint32_t * ) = fd_ed25519_gpu_txn_claims;
int (*p_try)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *, unsigned long * )
  = fd_ed25519_gpu_try_submit_txns;
int (*p_sub)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *, unsigned long * )
  = fd_ed25519_gpu_submit_txns;
int (*p_poll)( fd_ed25519_gpu_t *, unsigned long, fd_ed25519_gpu_txn_result_t *, int *, int ) = fd_ed25519_gpu_poll_txns;
unsigned long (*p_al)( fd_ed25519_gpu_t * ) = fd_ed25519_gpu_txn_ring_allocs;
int (*p_tm)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_txn_t const *,
             fd_ed25519_gpu_txn_result_t *, float * ) = fd_ed25519_gpu_txn_ring_timed;
int keep = FD_ED25519_GPU_POLL_KEEP;
"""


def test_header_is_c(tmp_path):
    src = tmp_path / "ring_abi.c"
    src.write_text(PROTOS)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "ring_abi.o")], check=True, capture_output=True)


def test_symbols_and_python_names():
    L = fa.lib()
    for s in SYMBOLS + ["fd_ed25519_gpu_txn_ring_allocs", "fd_ed25519_gpu_txn_ring_timed"]:
        assert hasattr(L, s), s
    for m in ("submit_txns", "try_submit_txns", "poll_txns"):
        assert callable(getattr(fa.Engine, m))
    assert callable(fa.txn_claims)


def test_null_engine_is_err_arg_and_writes_nothing():
    L = fa.lib()
    buf = np.full(256, 1, np.uint8)
    t = np.array([(0, 100)], fa.TXN_DTYPE)
    res = np.zeros(2, fa.TXN_RESULT_DTYPE)
    codes = np.full(4, 77, np.int32)
    ticket = ctypes.c_ulong(7)
    assert L.fd_ed25519_gpu_try_submit_txns(None, 1, P(buf), 256, P(t), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_submit_txns(None, 1, P(buf), 256, P(t), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_poll_txns(None, 1, P(res), P(codes), 1) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_poll_txns(None, 1, P(res), P(codes), 0) == fa.ERR_ARG
    ms = np.full(2, 5.0, np.float32)
    assert L.fd_ed25519_gpu_txn_ring_timed(None, 1, P(buf), 256, P(t), P(res), P(ms)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_txn_ring_allocs(None) == 0
    assert ticket.value == 7 and not res.view(np.uint8).any() and (codes == 77).all() and (ms == 5.0).all()
    assert (buf == 1).all() and t.tolist() == [(0, 100)]


def test_claims_need_no_engine_and_nothing_else_works_without_a_device():
    """the host routine is pure; with no device there is no engine to submit to, and
    making one fails with a message, as the existing entry points do"""
    blob = np.array([3, 0, 0, 0], np.uint8)
    bases, n_sig = fa.txn_claims(blob, np.array([(0, 4), (1, 3), (0, 5)], fa.TXN_DTYPE))
    assert bases.tolist() == [0, 3, 3, 3] and n_sig == 3
    if fa.device_count() == 0:
        assert fa.lib().fd_ed25519_gpu_new(0, 16, 4096) is None
        assert fa.last_error()
        with pytest.raises(fa.EngineError):
            fa.Engine(0, 16, 4096)
