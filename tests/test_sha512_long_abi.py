"""The long SHA-512 / SHA-384 path's C ABI (include/fd_sha512_gpu.h) without a
device: the symbols are there, no device means no digest (there is no CPU
fallback), the geometry diagnostic is pure arithmetic, and the verify
kernels' build id did not move with the new kernel unit."""
import ctypes

import firedancer_amd as fa


def test_symbols_exported():
    L = fa.lib()
    for n in ("fd_ed25519_gpu_sha512_ptrs", "fd_sha512_gpu_long_geometry", "fd_sha512_gpu_batch_fini"):
        assert hasattr(L, n), n
    assert hasattr(fa.Engine, "sha512_any")


def test_no_device_no_digest():
    if fa.device_count():
        return                           # the GPU suite covers the device (tests/test_gpu_sha512_long.py)
    L = fa.lib()
    msg = ctypes.create_string_buffer(b"abc", 3)
    ptrs = (ctypes.c_void_p * 1)(ctypes.cast(msg, ctypes.c_void_p))
    sz = (ctypes.c_ulong * 1)(3)
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    for is384 in (0, 1):
        assert L.fd_ed25519_gpu_sha512_ptrs(None, 1, ptrs, sz, out, is384) == fa.ERR_GPU
        assert out.raw == b"\xaa" * 64
    assert L.fd_ed25519_gpu_sha512_ptrs(None, 0, None, None, None, 0) == fa.ERR_GPU
    assert L.fd_sha512_gpu_batch_new(None, 0) is None
    assert L.fd_sha512_gpu_batch_new(None, 1) is None


def test_geometry_needs_no_device():
    # the shipped geometry: the blob is one buffer, a message costs 128 C + 16 bytes of it
    assert fa.sha512_long_geometry(144, 64, 1) == (1, 1)        # one block and its piece entry
    assert fa.sha512_long_geometry(143, 64, 1) is None          # the one failure: not even one block
    assert fa.sha512_long_geometry(287, 64, 1) == (1, 2)
    G, C = fa.sha512_long_geometry(2048, 64, 1)
    assert G == 2048 // 144 and C == (2048 - 16) // 128
    assert fa.sha512_long_geometry(2048, 64, G) == (G, 1)
    assert fa.sha512_long_geometry(2048, 64, G + 1) is None
    assert fa.sha512_long_geometry(1 << 26, 1 << 16, 1)[0] == 4096   # capped as the verify long path caps its groups
    assert fa.sha512_long_geometry(1 << 26, 100, 1)[0] == 100


def test_verify_kernels_id_unchanged():
    assert fa.kernels_id() == "f8cd592cbcd9b28d"
