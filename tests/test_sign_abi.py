"""The signing ABI (include/fd_ed25519_gpu_sign.h): the header is C, the
symbols are exported, and malformed calls are refused before anything
touches a device."""
import ctypes
import os
import subprocess

import numpy as np

import firedancer_amd as fa
from conftest import P, ROOT

SYMBOLS = ["fd_ed25519_gpu_public_packed", "fd_ed25519_gpu_sign_packed", "fd_ed25519_gpu_sign_dev",
           "fd_ed25519_gpu_sign_batch", "fd_ed25519_sign_batch_gpu", "fd_ed25519_gpu_debug_sign_op"]


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "fd_ed25519_gpu_sign.h"\n'
                   "_Static_assert( sizeof(fd_ed25519_gpu_sign_desc_t) == 16, \"as fd_ed25519_gpu_desc_t\" );\n"
                   "_Static_assert( sizeof(fd_ed25519_gpu_sign_desc_t) == sizeof(fd_ed25519_gpu_desc_t), \"one staging layout\" );\n"
                   "int (*p_sign)( fd_ed25519_gpu_t *, unsigned long, void const *, unsigned long, fd_ed25519_gpu_sign_desc_t const *,\n"
                   "               void *, void *, int * ) = fd_ed25519_gpu_sign_packed;\n"
                   "int (*p_pub)( fd_ed25519_gpu_t *, unsigned long, void const *, void * ) = fd_ed25519_gpu_public_packed;\n"
                   "unsigned derive = FD_ED25519_GPU_SIGN_DERIVE;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_symbols_exported():
    L = fa.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert fa.SIGN_DESC_DTYPE.itemsize == 16 and fa.SIGN_DERIVE == 0xFFFFFFFF
    for m in ("sign_packed", "public_from_seeds", "sign_dev", "debug_sign_op"):
        assert callable(getattr(fa.Engine, m))
    assert callable(fa.sign_batch_gpu)


def test_null_engine_is_err_arg():
    """no engine: every entry point that takes one answers ERR_ARG at once (no device is opened)"""
    L = fa.lib()
    buf = np.zeros(256, np.uint8)
    d = np.zeros(1, fa.SIGN_DESC_DTYPE)
    code = np.zeros(1, np.int32)
    assert L.fd_ed25519_gpu_sign_packed(None, 1, P(buf), 128, P(d), P(buf), None, P(code)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_public_packed(None, 1, P(buf), P(buf)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_sign_dev(None, 1, P(buf), 128, P(d), P(buf), None, P(code), None) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_debug_sign_op(None, 0, 1, P(buf), None, None, P(buf)) == fa.ERR_ARG
    assert not buf.any() and code[0] == 0
