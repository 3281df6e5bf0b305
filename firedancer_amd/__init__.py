"""firedancer_amd -- MI355X-native Ed25519 signature verification engine.

Drop-in for tinydancer-io/firedancer's sigverify hot path
(``fd_ed25519_verify``, src/ballet/ed25519/fd_ed25519.h:96-101).  The
product is the C-ABI shared library ``libfd_ed25519_gpu.so`` (HIP kernels
for gfx950 + host runtime, declared in ``include/fd_ed25519_gpu.h``).
This module is a thin ctypes mirror of that ABI for tests, benchmarks
and Python callers; it never verifies anything itself and raises if the
library or a gfx950 device is missing.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_ED25519_LIB") or os.path.join(_HERE, "libfd_ed25519_gpu.so")  # override: experiments only

SUCCESS = 0
ERR_SIG = -1
ERR_PUBKEY = -2
ERR_MSG = -3
ERR_ARG = -16
ERR_GPU = -17
ERR_TXN = -18       # FD_ED25519_ERR_TXN (fd_ed25519_gpu_txn.h): fd_txn_parse would return 0

MODE_AVX = 0        # reference AVX2 build semantics (default)
MODE_PORTABLE = 1   # reference FD_HAS_AVX=0 build semantics
MODE_STRICT = 2     # AVX checks with Q1-Q3 fixed (no reference build)


DESC_DTYPE = np.dtype([("sig_off", "<u4"), ("pub_off", "<u4"), ("msg_off", "<u4"), ("msg_sz", "<u4")])
# fd_ed25519_gpu_sign_desc_t; pub_off = SIGN_DERIVE: the key is derived from the seed on the device
SIGN_DESC_DTYPE = np.dtype([("seed_off", "<u4"), ("pub_off", "<u4"), ("msg_off", "<u4"), ("msg_sz", "<u4")])
SIGN_DERIVE = 0xFFFFFFFF
# fd_ed25519_gpu_txn_t: one transaction, payload = blob[off, off+sz)
TXN_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4")])
# fd_ed25519_gpu_txn_result_t
TXN_RESULT_DTYPE = np.dtype([("status", "<i4"), ("sig_base", "<u4"), ("tag", "<u8"), ("footprint", "<u2"),
                             ("reject_line", "<u2"), ("sig_cnt", "u1"), ("version", "u1"), ("_pad", "u1", (2,))])

_lib = None


# fd_poh_gpu_entry_t (fd_poh_gpu.h): one Proof-of-History entry, 112 bytes
POH_ENTRY_DTYPE = np.dtype([("start", "u1", (32,)), ("mixin", "u1", (32,)), ("expect", "u1", (32,)),
                            ("n", "<u8"), ("flags", "<u4"), ("_pad", "<u4")])
POH_MIXIN = 1        # FD_POH_GPU_MIXIN
POH_ERR_HASH = -1    # FD_POH_ERR_HASH: the chain does not reach expect
POH_CHUNK_DEFAULT = 16384

# fd_bmtree_gpu_leaf_t (fd_bmtree_gpu.h): a leaf is blob[off, off+sz)
BMTREE_LEAF_DTYPE = np.dtype([("off", "<u4"), ("sz", "<u4")])
BMTREE_LEAVES_ARE_NODES = 1   # FD_BMTREE_GPU_LEAVES_ARE_NODES
BMTREE_LEAF_SZ_MAX = 65535    # FD_BMTREE_GPU_LEAF_SZ_MAX
# fd_bmtree_gpu_proof_t: a leaf, its inclusion proof and where the walk should end, all offsets into one blob
BMTREE_PROOF_DTYPE = np.dtype([("leaf_off", "<u4"), ("leaf_sz", "<u4"), ("proof_off", "<u4"), ("idx", "<u4"), ("leaf_cnt", "<u4"),
                               ("depth", "<u4"), ("expect_off", "<u4"), ("flags", "<u4")])
BMTREE_PROOF_EXPECT = 1       # FD_BMTREE_GPU_PROOF_EXPECT
BMTREE_ERR_PROOF = -1         # FD_BMTREE_ERR_PROOF: the walk does not reach the expected root


class Stages:
    """what Engine.debug_stages read back from one launch"""


class EngineError(RuntimeError):
    pass


def _share_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own
    libamdhip64 (soname libamdhip64.so.7) and links it by file name, so if
    our library (which needs libamdhip64.so.7) were loaded first, torch
    would later load a second runtime and fail to initialise the GPU.
    Importing torch first makes the loader satisfy our dependency with
    torch's already-loaded copy.  Without torch, /opt/rocm's runtime is
    used."""
    if os.environ.get("FD_ED25519_NO_TORCH"):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib() -> ctypes.CDLL:
    """Load the product library (fails loudly when it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} missing: run __graft_entry__.build() (make -C firedancer_amd)")
        _share_hip_runtime()
        L = ctypes.CDLL(LIB_PATH)
        vp, ul, ip = ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int
        L.fd_ed25519_verify.argtypes = [vp, ul, vp, vp, vp]
        L.fd_ed25519_verify.restype = ip
        L.fd_ed25519_strerror.argtypes = [ip]
        L.fd_ed25519_strerror.restype = ctypes.c_char_p
        L.fd_ed25519_verify_batch.argtypes = [ul, vp, vp, vp, vp, vp]
        L.fd_ed25519_verify_batch.restype = ip
        L.fd_ed25519_verify_batch_single_msg.argtypes = [vp, ul, vp, vp, ul, vp]
        L.fd_ed25519_verify_batch_single_msg.restype = ip
        L.fd_ed25519_gpu_new.argtypes = [ip, ul, ul]
        L.fd_ed25519_gpu_new.restype = vp
        L.fd_ed25519_gpu_delete.argtypes = [vp]
        L.fd_ed25519_gpu_delete.restype = None
        L.fd_ed25519_gpu_verify_packed.argtypes = [vp, ul, vp, ul, vp, vp]
        L.fd_ed25519_gpu_verify_packed.restype = ip
        L.fd_ed25519_gpu_verify_dev.argtypes = [vp, ul, vp, ul, vp, vp, vp]
        L.fd_ed25519_gpu_verify_dev.restype = ip
        L.fd_ed25519_gpu_verify_dev_ex.argtypes = [vp, ul, vp, ul, vp, vp, vp, ip]
        L.fd_ed25519_gpu_verify_dev_ex.restype = ip
        L.fd_ed25519_gpu_verify_dev_timed.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp]
        L.fd_ed25519_gpu_verify_dev_timed.restype = ip
        L.fd_ed25519_gpu_dev_stats_begin.argtypes = [vp]
        L.fd_ed25519_gpu_dev_stats_begin.restype = ip
        L.fd_ed25519_gpu_dev_stats_end.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_ulong)]
        L.fd_ed25519_gpu_dev_stats_end.restype = ip
        L.fd_ed25519_gpu_dsm_clock.argtypes = [vp, ip, vp]
        L.fd_ed25519_gpu_dsm_clock.restype = ip
        L.fd_ed25519_gpu_kernel_cnt.argtypes = []
        L.fd_ed25519_gpu_kernel_cnt.restype = ip
        L.fd_ed25519_public_batch.argtypes = [ul, vp, vp, ip]
        L.fd_ed25519_public_batch.restype = None
        L.fd_ed25519_gpu_submit.argtypes = [vp, ul, vp, ul, vp, ctypes.POINTER(ctypes.c_ulong)]
        L.fd_ed25519_gpu_submit.restype = ip
        L.fd_ed25519_gpu_try_submit.argtypes = [vp, ul, vp, ul, vp, ctypes.POINTER(ctypes.c_ulong)]
        L.fd_ed25519_gpu_try_submit.restype = ip
        L.fd_ed25519_gpu_try_submit2.argtypes = [vp, ul, vp, ul, vp, ul, vp, ctypes.POINTER(ctypes.c_ulong)]
        L.fd_ed25519_gpu_try_submit2.restype = ip
        L.fd_ed25519_gpu_feeder_synth.argtypes = [vp, vp, ul, vp, ul, ul, vp, ul, ul, ip, ul, vp, vp]
        L.fd_ed25519_gpu_feeder_synth.restype = ip
        L.fd_ed25519_gpu_poll.argtypes = [vp, ul, vp, ip]
        L.fd_ed25519_gpu_poll.restype = ip
        L.fd_ed25519_gpu_depth.argtypes = [vp]
        L.fd_ed25519_gpu_depth.restype = ip
        L.fd_ed25519_gpu_set_timeout.argtypes = [vp, ctypes.c_long]
        L.fd_ed25519_gpu_set_timeout.restype = ip
        L.fd_ed25519_gpu_timeout.argtypes = [vp]
        L.fd_ed25519_gpu_timeout.restype = ctypes.c_long
        L.fd_ed25519_gpu_wait_selftest.argtypes = [ctypes.c_long, ctypes.c_long]
        L.fd_ed25519_gpu_wait_selftest.restype = ip
        L.fd_ed25519_gpu_device.argtypes = [vp]
        L.fd_ed25519_gpu_device.restype = ip
        L.fd_ed25519_gpu_last_error.argtypes = []
        L.fd_ed25519_gpu_last_error.restype = ctypes.c_char_p
        L.fd_ed25519_gpu_device_cnt.argtypes = []
        L.fd_ed25519_gpu_device_cnt.restype = ip
        L.fd_ed25519_public_from_private.argtypes = [vp, vp, vp]
        L.fd_ed25519_public_from_private.restype = vp
        L.fd_ed25519_sign.argtypes = [vp, vp, ul, vp, vp, vp]
        L.fd_ed25519_sign.restype = vp
        L.fd_ed25519_sign_batch.argtypes = [ul, vp, vp, vp, vp, vp, vp, ip]
        L.fd_ed25519_sign_batch.restype = None
        L.fd_ed25519_gpu_new_ex.argtypes = [ip, ul, ul, ip]
        L.fd_ed25519_gpu_new_ex.restype = vp
        L.fd_ed25519_gpu_max_sigs.argtypes = [vp]
        L.fd_ed25519_gpu_max_sigs.restype = ul
        L.fd_ed25519_gpu_max_blob.argtypes = [vp]
        L.fd_ed25519_gpu_max_blob.restype = ul
        L.fd_ed25519_gpu_verify_ptrs.argtypes = [vp, ul, vp, vp, vp, vp, vp]
        L.fd_ed25519_gpu_verify_ptrs.restype = ip
        L.fd_ed25519_gpu_stage.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
        L.fd_ed25519_gpu_stage.restype = ip
        L.fd_ed25519_gpu_unstage.argtypes = [vp, vp]
        L.fd_ed25519_gpu_unstage.restype = None
        L.fd_txn_parse.argtypes = [vp, ul, vp, vp]
        L.fd_txn_parse.restype = ul
        L.fd_verify_tile_new.argtypes = [vp, vp, vp, vp]
        L.fd_verify_tile_new.restype = vp
        L.fd_verify_tile_delete.argtypes = [vp]
        L.fd_verify_tile_delete.restype = None
        L.fd_verify_tile_rx.argtypes = [vp, vp, ul, ul, ul]
        L.fd_verify_tile_rx.restype = ip
        L.fd_verify_tile_rx_burst.argtypes = [vp, vp, vp, vp, vp, vp, ul]
        L.fd_verify_tile_rx_burst.restype = ip
        L.fd_verify_tile_rx_burst_now.argtypes = [vp, vp, vp, vp, ul]
        L.fd_verify_tile_rx_burst_now.restype = ip
        L.fd_verify_tile_new_multi.argtypes = [vp, ul, vp, vp, vp]
        L.fd_verify_tile_new_multi.restype = vp
        L.fd_verify_tile_new_inplace.argtypes = [vp, vp, vp, ul, vp, vp]
        L.fd_verify_tile_new_inplace.restype = vp
        L.fd_verify_tile_new_multi_inplace.argtypes = [vp, ul, vp, vp, ul, vp, vp]
        L.fd_verify_tile_new_multi_inplace.restype = vp
        L.fd_verify_tile_held.argtypes = [vp]
        L.fd_verify_tile_held.restype = ul
        L.fd_verify_tile_service.argtypes = [vp, ip]
        L.fd_verify_tile_service.restype = ip
        L.fd_verify_tile_diag.argtypes = [vp, vp]
        L.fd_verify_tile_diag.restype = None
        L.fd_vt_tcache_new.argtypes = [ul, ul]
        L.fd_vt_tcache_new.restype = vp
        L.fd_vt_tcache_insert.argtypes = [vp, ul]
        L.fd_vt_tcache_insert.restype = ip
        L.fd_vt_tcache_delete.argtypes = [vp]
        L.fd_vt_tcache_delete.restype = None
        L.fd_ed25519_gpu_debug_k.argtypes = [vp, ul, vp, ul, vp, vp, vp]
        L.fd_ed25519_gpu_debug_k.restype = ip
        L.fd_ed25519_gpu_debug_verify_dig.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, vp]
        L.fd_ed25519_gpu_debug_verify_dig.restype = ip
        L.fd_ed25519_gpu_debug_stages.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.fd_ed25519_gpu_debug_stages.restype = ip
        L.fd_ed25519_gpu_debug_fe.argtypes = [vp, ip, ul, vp, vp, vp]
        L.fd_ed25519_gpu_debug_fe.restype = ip
        L.fd_ed25519_gpu_sha512_packed.argtypes = [vp, ul, vp, ul, vp, vp, ip]
        L.fd_ed25519_gpu_sha512_packed.restype = ip
        L.fd_ed25519_gpu_default.argtypes = []
        L.fd_ed25519_gpu_default.restype = vp
        L.fd_ed25519_gpu_set_mode.argtypes = [vp, ip]
        L.fd_ed25519_gpu_set_mode.restype = ip
        L.fd_ed25519_gpu_mode.argtypes = [vp]
        L.fd_ed25519_gpu_mode.restype = ip
        L.fd_ed25519_gpu_set_dsm_pool_min.argtypes = [vp, ul]
        L.fd_ed25519_gpu_set_dsm_pool_min.restype = ip
        L.fd_ed25519_gpu_dsm_pool_min.argtypes = [vp]
        L.fd_ed25519_gpu_dsm_pool_min.restype = ul
        L.fd_ed25519_gpu_set_dsm_quad_max.argtypes = [vp, ul]
        L.fd_ed25519_gpu_set_dsm_quad_max.restype = ip
        L.fd_ed25519_gpu_dsm_quad_max.argtypes = [vp]
        L.fd_ed25519_gpu_dsm_quad_max.restype = ul
        L.fd_ed25519_gpu_set_dsm_oct_max.argtypes = [vp, ul]
        L.fd_ed25519_gpu_set_dsm_oct_max.restype = ip
        L.fd_ed25519_gpu_dsm_oct_max.argtypes = [vp]
        L.fd_ed25519_gpu_dsm_oct_max.restype = ul
        L.fd_ed25519_gpu_multi_new.argtypes = [vp, ip, ul, ul]
        L.fd_ed25519_gpu_multi_new.restype = vp
        L.fd_ed25519_gpu_multi_delete.argtypes = [vp]
        L.fd_ed25519_gpu_multi_delete.restype = None
        L.fd_ed25519_gpu_multi_cnt.argtypes = [vp]
        L.fd_ed25519_gpu_multi_cnt.restype = ip
        L.fd_ed25519_gpu_multi_engine.argtypes = [vp, ip]
        L.fd_ed25519_gpu_multi_engine.restype = vp
        L.fd_ed25519_gpu_multi_verify_packed.argtypes = [vp, ul, vp, ul, vp, vp]
        L.fd_ed25519_gpu_multi_verify_packed.restype = ip
        L.fd_ed25519_codes_to_bitmap.argtypes = [ul, vp, vp]
        L.fd_ed25519_codes_to_bitmap.restype = None
        L.fd_ed25519_gpu_set_cu_groups.argtypes = [vp, ip]
        L.fd_ed25519_gpu_set_cu_groups.restype = ip
        L.fd_ed25519_gpu_cu_groups.argtypes = [vp]
        L.fd_ed25519_gpu_cu_groups.restype = ip
        L.fd_ed25519_gpu_register.argtypes = [vp, vp, ul]
        L.fd_ed25519_gpu_register.restype = ip
        L.fd_ed25519_gpu_unregister.argtypes = [vp, vp]
        L.fd_ed25519_gpu_unregister.restype = ip
        L.fd_ed25519_gpu_feeder_new.argtypes = [vp, ip]
        L.fd_ed25519_gpu_feeder_new.restype = vp
        L.fd_ed25519_gpu_feeder_delete.argtypes = [vp]
        L.fd_ed25519_gpu_feeder_delete.restype = None
        L.fd_ed25519_gpu_device_numa_node.argtypes = [ip]
        L.fd_ed25519_gpu_device_numa_node.restype = ip
        L.fd_ed25519_gpu_feeder_numa_node.argtypes = [vp]
        L.fd_ed25519_gpu_feeder_numa_node.restype = ip
        L.fd_ed25519_gpu_feeder_push.argtypes = [vp, vp]
        L.fd_ed25519_gpu_feeder_push.restype = ip
        L.fd_ed25519_gpu_job_wait.argtypes = [vp, ctypes.c_long]
        L.fd_ed25519_gpu_job_wait.restype = ip
        L.fd_ed25519_gpu_multi_new_ex.argtypes = [vp, ip, ul, ul, ip]
        L.fd_ed25519_gpu_multi_new_ex.restype = vp
        L.fd_ed25519_gpu_multi_feeder.argtypes = [vp, ip]
        L.fd_ed25519_gpu_multi_feeder.restype = vp
        L.fd_ed25519_gpu_sha512_ptrs.argtypes = [vp, ul, vp, vp, vp, ip]
        L.fd_ed25519_gpu_sha512_ptrs.restype = ip
        L.fd_sha512_gpu_long_geometry.argtypes = [ul, ul, ul, ctypes.POINTER(ctypes.c_ulong), ctypes.POINTER(ctypes.c_ulong)]
        L.fd_sha512_gpu_long_geometry.restype = ip
        L.fd_sha512_gpu_batch_new.argtypes = [vp, ip]
        L.fd_sha512_gpu_batch_new.restype = vp
        L.fd_sha512_gpu_batch_delete.argtypes = [vp]
        L.fd_sha512_gpu_batch_delete.restype = None
        L.fd_sha512_gpu_batch_init.argtypes = [vp]
        L.fd_sha512_gpu_batch_init.restype = vp
        L.fd_sha512_gpu_batch_add.argtypes = [vp, vp, ul, vp]
        L.fd_sha512_gpu_batch_add.restype = vp
        L.fd_sha512_gpu_batch_fini.argtypes = [vp]
        L.fd_sha512_gpu_batch_fini.restype = vp
        L.fd_sha512_gpu_batch_abort.argtypes = [vp]
        L.fd_sha512_gpu_batch_abort.restype = vp
        L.fd_ed25519_gpu_public_packed.argtypes = [vp, ul, vp, vp]
        L.fd_ed25519_gpu_public_packed.restype = ip
        L.fd_ed25519_gpu_sign_packed.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp]
        L.fd_ed25519_gpu_sign_packed.restype = ip
        L.fd_ed25519_gpu_sign_dev.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, vp]
        L.fd_ed25519_gpu_sign_dev.restype = ip
        L.fd_ed25519_gpu_sign_batch.argtypes = [vp, ul, vp, vp, vp, vp, vp, vp, ip]
        L.fd_ed25519_gpu_sign_batch.restype = ip
        L.fd_ed25519_sign_batch_gpu.argtypes = [ul, vp, vp, vp, vp, vp, vp, ip]
        L.fd_ed25519_sign_batch_gpu.restype = ip
        L.fd_ed25519_gpu_debug_sign_op.argtypes = [vp, ip, ul, vp, vp, vp, vp]
        L.fd_ed25519_gpu_debug_sign_op.restype = ip
        L.fd_ed25519_gpu_sign_set_batch_inv.argtypes = [ip]
        L.fd_ed25519_gpu_sign_set_batch_inv.restype = ip
        L.fd_ed25519_gpu_txns_reserve.argtypes = [vp, ul]
        L.fd_ed25519_gpu_txns_reserve.restype = ip
        L.fd_ed25519_gpu_verify_txns_dev.argtypes = [vp, ul, vp, ul, vp, ul, vp, vp, vp, ul, vp]
        L.fd_ed25519_gpu_verify_txns_dev.restype = ip
        L.fd_ed25519_gpu_verify_txns_dev_timed.argtypes = [vp, ul, vp, ul, vp, ul, vp, vp, vp, ul, vp, vp]
        L.fd_ed25519_gpu_verify_txns_dev_timed.restype = ip
        L.fd_ed25519_gpu_verify_txns_packed.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, ul]
        L.fd_ed25519_gpu_verify_txns_packed.restype = ip
        L.fd_ed25519_gpu_debug_txn_descs.argtypes = [vp, ul, vp, ul, vp, ul, vp, ctypes.POINTER(ul), vp]
        L.fd_ed25519_gpu_debug_txn_descs.restype = ip
        L.fd_ed25519_gpu_txn_claims.argtypes = [vp, ul, vp, ul, vp]
        L.fd_ed25519_gpu_txn_claims.restype = ul
        L.fd_ed25519_gpu_try_submit_txns.argtypes = [vp, ul, vp, ul, vp, ctypes.POINTER(ul)]
        L.fd_ed25519_gpu_try_submit_txns.restype = ip
        L.fd_ed25519_gpu_submit_txns.argtypes = [vp, ul, vp, ul, vp, ctypes.POINTER(ul)]
        L.fd_ed25519_gpu_submit_txns.restype = ip
        L.fd_ed25519_gpu_poll_txns.argtypes = [vp, ul, vp, vp, ip]
        L.fd_ed25519_gpu_poll_txns.restype = ip
        L.fd_ed25519_gpu_txn_ring_allocs.argtypes = [vp]
        L.fd_ed25519_gpu_txn_ring_allocs.restype = ul
        L.fd_ed25519_gpu_txn_ring_timed.argtypes = [vp, ul, vp, ul, vp, vp, vp]
        L.fd_ed25519_gpu_txn_ring_timed.restype = ip
        L.fd_poh_append.argtypes = [vp, ul]
        L.fd_poh_append.restype = vp
        L.fd_poh_mixin.argtypes = [vp, vp]
        L.fd_poh_mixin.restype = vp
        L.fd_poh_verify_batch.argtypes = [ul, vp, ul, vp, vp, ip]
        L.fd_poh_verify_batch.restype = ip
        L.fd_poh_gpu_verify_packed.argtypes = [vp, ul, vp, ul, vp, vp]
        L.fd_poh_gpu_verify_packed.restype = ip
        L.fd_poh_gpu_verify_dev.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp]
        L.fd_poh_gpu_verify_dev.restype = ip
        L.fd_poh_gpu_work_sz.argtypes = [ul]
        L.fd_poh_gpu_work_sz.restype = ul
        L.fd_poh_gpu_chain.argtypes = [ul, vp, vp, vp]
        L.fd_poh_gpu_chain.restype = None
        L.fd_poh_gpu_debug_set_chunk.argtypes = [vp, ul]
        L.fd_poh_gpu_debug_set_chunk.restype = ip
        L.fd_poh_gpu_debug_set_sort.argtypes = [vp, ip]
        L.fd_poh_gpu_debug_set_sort.restype = ip
        L.fd_poh_gpu_chunk.argtypes = [vp]
        L.fd_poh_gpu_chunk.restype = ul
        u = ctypes.c_uint
        L.fd_poh_gpu_verify_entries_packed.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, vp, ul, ul]
        L.fd_poh_gpu_verify_entries_packed.restype = ip
        L.fd_poh_gpu_verify_entries_dev.argtypes = [vp, ul, vp, ul, vp, vp, vp, vp, ul, vp, vp, ul, ul, vp, vp]
        L.fd_poh_gpu_verify_entries_dev.restype = ip
        L.fd_poh_gpu_entries_work_sz.argtypes = [ul, ul]
        L.fd_poh_gpu_entries_work_sz.restype = ul
        for w in ("20", "32"):
            f = getattr(L, f"fd_bmtree{w}_hash_leaf")
            f.argtypes, f.restype = [vp, vp, ul], vp
            for name in ("commit_align", "commit_footprint"):
                f = getattr(L, f"fd_bmtree{w}_{name}")
                f.argtypes, f.restype = [], ul
            f = getattr(L, f"fd_bmtree{w}_commit_init")
            f.argtypes, f.restype = [vp], vp
            f = getattr(L, f"fd_bmtree{w}_commit_leaf_cnt")
            f.argtypes, f.restype = [vp], ul
            f = getattr(L, f"fd_bmtree{w}_commit_append")
            f.argtypes, f.restype = [vp, vp, ul], vp
            f = getattr(L, f"fd_bmtree{w}_commit_fini")
            f.argtypes, f.restype = [vp], vp
        L.fd_bmtree_roots_batch.argtypes = [u, u, ul, vp, vp, vp, ul, ul, vp, vp, ip]
        L.fd_bmtree_roots_batch.restype = ip
        L.fd_bmtree_gpu_roots_packed.argtypes = [vp, u, u, ul, vp, vp, vp, ul, ul, vp, vp]
        L.fd_bmtree_gpu_roots_packed.restype = ip
        L.fd_bmtree_gpu_roots_dev.argtypes = [vp, u, u, ul, vp, ul, vp, vp, ul, ul, vp, ul, vp, vp, vp]
        L.fd_bmtree_gpu_roots_dev.restype = ip
        L.fd_bmtree_proofs_batch.argtypes = [u, u, ul, vp, vp, vp, ul, ul, vp, vp, vp, ul, ip]
        L.fd_bmtree_proofs_batch.restype = ip
        L.fd_bmtree_gpu_proofs_packed.argtypes = [vp, u, u, ul, vp, vp, vp, ul, ul, vp, vp, vp, ul]
        L.fd_bmtree_gpu_proofs_packed.restype = ip
        L.fd_bmtree_gpu_proofs_dev.argtypes = [vp, u, u, ul, vp, ul, vp, vp, ul, ul, vp, ul, vp, ul, vp, vp, vp]
        L.fd_bmtree_gpu_proofs_dev.restype = ip
        L.fd_bmtree_from_proofs_batch.argtypes = [u, u, ul, vp, vp, ul, ul, vp, vp, ip]
        L.fd_bmtree_from_proofs_batch.restype = ip
        L.fd_bmtree_gpu_from_proofs_packed.argtypes = [vp, u, u, ul, vp, vp, ul, ul, vp, vp]
        L.fd_bmtree_gpu_from_proofs_packed.restype = ip
        L.fd_bmtree_gpu_from_proofs_dev.argtypes = [vp, u, u, ul, vp, vp, ul, ul, vp, ul, vp, vp]
        L.fd_bmtree_gpu_from_proofs_dev.restype = ip
        L.fd_bmtree_gpu_work_sz.argtypes = [ul, ul]
        L.fd_bmtree_gpu_work_sz.restype = ul
        L.fd_bmtree_gpu_merge_passes.argtypes = [u, ul, vp]
        L.fd_bmtree_gpu_merge_passes.restype = ul
        _lib = L
    return _lib


def _p(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


def strerror(err: int) -> str:
    return lib().fd_ed25519_strerror(err).decode()


def last_error() -> str:
    return (lib().fd_ed25519_gpu_last_error() or b"").decode()


def sha512_long_geometry(max_blob: int, max_sigs: int, m: int = 1):
    """fd_sha512_gpu_long_geometry: (G, C) of the long hash path, or None
    where m is not in [1, G] (G 0: a blob that cannot hold one block)."""
    G, C = ctypes.c_ulong(0), ctypes.c_ulong(0)
    if lib().fd_sha512_gpu_long_geometry(max_blob, max_sigs, m, ctypes.byref(G), ctypes.byref(C)):
        return None
    return G.value, C.value


def _sha512_ptrs(handle, msgs, is384: bool = False) -> list:
    """fd_ed25519_gpu_sha512_ptrs on an engine handle (None: the default engine)"""
    n = len(msgs)
    keep = [m if isinstance(m, np.ndarray) else np.frombuffer(bytes(m), np.uint8) for m in msgs]
    MP = ctypes.c_void_p * max(n, 1)
    mp = MP(*[m.ctypes.data if len(m) else None for m in keep])
    sz = (ctypes.c_ulong * max(n, 1))(*[len(m) for m in keep])
    hsz = 48 if is384 else 64
    out = np.zeros(max(n, 1) * hsz, np.uint8)
    err = lib().fd_ed25519_gpu_sha512_ptrs(handle, n, mp, sz, _p(out), 1 if is384 else 0)
    if err:
        raise EngineError(f"sha512_ptrs: {strerror(err)}: {last_error()}")
    return [out[i * hsz:(i + 1) * hsz].tobytes() for i in range(n)]


class Engine:
    """One verification engine bound to one gfx950 device (fd_ed25519_gpu_t)."""

    def __init__(self, device: int = 0, max_sigs: int = 1 << 16, max_blob: int = 1 << 26, depth: int = 3):
        L = lib()
        self._h = L.fd_ed25519_gpu_new_ex(device, max_sigs, max_blob, depth)
        if not self._h:
            raise EngineError(f"fd_ed25519_gpu_new(device={device}) failed: {last_error()}")
        self.device = device
        self.max_sigs = max_sigs
        self.max_blob = max_blob
        self._pending = {}
        self._pending_txns = {}     # ticket -> n_sig (the claimed total)
        self._registered = []

    def close(self):
        if self._h:
            lib().fd_ed25519_gpu_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_packed(self, blob: np.ndarray, desc: np.ndarray) -> np.ndarray:
        """Host batch in, host codes out (synchronous)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        out = np.empty(len(desc), dtype=np.int32)
        err = lib().fd_ed25519_gpu_verify_packed(self._h, len(desc), _p(blob), blob.nbytes, _p(desc), _p(out))
        if err:
            raise EngineError(f"verify_packed: {strerror(err)}: {last_error()}")
        return out

    def verify_ptrs(self, msgs, sigs, pubs) -> tuple[int, np.ndarray]:
        """fd_ed25519_gpu_verify_ptrs: fd_ed25519_verify_batch on this engine,
        messages of any length (past max_blob: the long path)."""
        n = len(msgs)
        keep = [m if isinstance(m, np.ndarray) else np.frombuffer(bytes(m), np.uint8) for m in msgs]
        sb = [ctypes.create_string_buffer(bytes(x), 64) for x in sigs]
        pb = [ctypes.create_string_buffer(bytes(x), 32) for x in pubs]
        MP = ctypes.c_void_p * max(n, 1)
        mp = MP(*[m.ctypes.data if len(m) else None for m in keep])
        sp = MP(*[ctypes.cast(b, ctypes.c_void_p) for b in sb])
        pp = MP(*[ctypes.cast(b, ctypes.c_void_p) for b in pb])
        sz = (ctypes.c_ulong * max(n, 1))(*[len(m) for m in keep])
        out = np.zeros(n, dtype=np.int32)
        r = lib().fd_ed25519_gpu_verify_ptrs(self._h, n, mp, sz, sp, pp, _p(out))
        if r in (ERR_ARG, ERR_GPU):
            raise EngineError(f"verify_ptrs: {strerror(r)}: {last_error()}")
        return r, out

    def verify_dev(self, n: int, d_blob: int, blob_sz: int, d_desc: int, d_out: int, stream: int = 0,
                   inputs_ready: bool = False) -> None:
        """Device-resident batch (raw device pointers, e.g. torch tensor .data_ptr());
        blob_sz = payload bytes at d_blob (descriptors are bounds-checked against it).
        inputs_ready: the inputs are already complete on the device (no ordering
        after work queued on `stream`), so successive launches overlap."""
        err = lib().fd_ed25519_gpu_verify_dev_ex(self._h, n, d_blob, blob_sz, d_desc, d_out, stream or None,
                                                 1 if inputs_ready else 0)
        if err:
            raise EngineError(f"verify_dev: {strerror(err)}: {last_error()}")

    KERNELS = ("fd_k_prep", "fd_k_decomp", "fd_k_dsm_setup", "fd_k_dsm_pool", "fd_k_dsm_final")

    def verify_dev_timed(self, n: int, d_blob: int, blob_sz: int, d_desc: int, d_out: int, stream: int = 0) -> np.ndarray:
        """verify_dev with per-kernel HIP-event durations (ms), in KERNELS order."""
        ms = np.zeros(lib().fd_ed25519_gpu_kernel_cnt(), np.float32)
        err = lib().fd_ed25519_gpu_verify_dev_timed(self._h, n, d_blob, blob_sz, d_desc, d_out, stream or None, _p(ms))
        if err:
            raise EngineError(f"verify_dev_timed: {strerror(err)}: {last_error()}")
        return ms

    def dev_stats_begin(self) -> None:
        """start timing each kernel of the following pipelined verify_dev launches"""
        if lib().fd_ed25519_gpu_dev_stats_begin(self._h):
            raise EngineError("dev_stats_begin")

    def dev_stats_end(self):
        """-> (per-kernel mean ms over the launches since begin, in KERNELS order; launches)"""
        ms = np.zeros(lib().fd_ed25519_gpu_kernel_cnt(), np.float32)
        cnt = ctypes.c_ulong(0)
        err = lib().fd_ed25519_gpu_dev_stats_end(self._h, _p(ms), ctypes.byref(cnt))
        if err:
            raise EngineError(f"dev_stats_end: {strerror(err)}: {last_error()}")
        return (ms / max(cnt.value, 1)).astype(np.float64), cnt.value

    def dsm_clock(self, clear: bool = False):
        """Shader clock the DSM kernels ran at on this engine's device since
        the last clear (fd_ed25519_gpu_dsm_clock): None after clear=True,
        else {"pool": {"waves", "ghz"}, "quad": {...}, "oct": {...}} (ghz None when no wave
        of that kernel ran).  Call with the device idle."""
        out = np.zeros(9, np.uint64)
        err = lib().fd_ed25519_gpu_dsm_clock(self._h, 1 if clear else 0, None if clear else _p(out))
        if err:
            raise EngineError(f"dsm_clock: {strerror(err)}: {last_error()}")
        if clear:
            return None
        def one(w, c, t):
            return {"waves": int(w), "ghz": (0.1 * float(c) / float(t)) if t else None,
                    "cycles_per_wave": float(c) / float(w) if w else None,
                    "us_per_wave": 0.01 * float(t) / float(w) if w else None}
        return {"pool": one(*out[0:3]), "quad": one(*out[3:6]), "oct": one(*out[6:9])}

    def submit(self, blob: np.ndarray, desc: np.ndarray) -> int:
        """Queue a batch on the pinned ring; returns its ticket."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        t = ctypes.c_ulong(0)
        err = lib().fd_ed25519_gpu_submit(self._h, len(desc), _p(blob), blob.nbytes, _p(desc), ctypes.byref(t))
        if err:
            raise EngineError(f"submit: {strerror(err)}: {last_error()}")
        self._pending[t.value] = len(desc)
        return t.value

    def poll(self, ticket: int, out: np.ndarray, block: bool = True) -> bool:
        """Collect a ticket's codes into out (int32, contiguous, >= the batch's
        signature count); False while the batch is in flight."""
        n = self._pending.get(ticket)
        if n is None:
            raise EngineError(f"poll: unknown ticket {ticket}")
        if not isinstance(out, np.ndarray) or out.dtype != np.int32 or not out.flags.c_contiguous or out.size < n:
            raise EngineError(f"poll: out must be a contiguous int32 array of >= {n} entries")
        r = lib().fd_ed25519_gpu_poll(self._h, ticket, _p(out), 1 if block else 0)
        if r < 0:
            raise EngineError(f"poll: {strerror(r)}: {last_error()}")
        if r == 1:
            del self._pending[ticket]
        return r == 1

    @property
    def timeout_ns(self) -> int:
        """bound on one blocking wait (ns; < 0 unbounded)"""
        return lib().fd_ed25519_gpu_timeout(self._h)

    @timeout_ns.setter
    def timeout_ns(self, ns: int) -> None:
        if lib().fd_ed25519_gpu_set_timeout(self._h, int(ns)):
            raise EngineError("set_timeout")

    def debug_k(self, blob: np.ndarray, desc: np.ndarray):
        """Diagnostics: (k[n,32], status[n]) from fd_k_prep -- k = SHA-512(R||A||M)
        mod L for signatures whose S check is pending (status 1), else zeros."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        k = np.zeros((len(desc), 32), np.uint8)
        st = np.zeros(len(desc), np.int32)
        err = lib().fd_ed25519_gpu_debug_k(self._h, len(desc), _p(blob), blob.nbytes, _p(desc), _p(k), _p(st))
        if err:
            raise EngineError(f"debug_k: {strerror(err)}: {last_error()}")
        return k, st

    def debug_verify_dig(self, blob: np.ndarray, desc: np.ndarray, dig: np.ndarray):
        """Diagnostics (fd_ed25519_gpu_debug_verify_dig): the verify pipeline with each
        signature's 64-byte digest given (dig, [n,64] uint8: what the reference
        feeds fd_ed25519_sc_reduce) in place of SHA-512(R||A||M), on the schedule
        the engine's mode and knobs give a batch of n -> (codes[n], k[n,32], status[n]);
        k and status as debug_k."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        dig = np.ascontiguousarray(dig, dtype=np.uint8)
        n = len(desc)
        if dig.size != 64 * n:
            raise EngineError(f"debug_verify_dig: dig holds {dig.size} bytes, not 64 per signature ({64 * n})")
        codes = np.zeros(n, np.int32)
        k = np.zeros((n, 32), np.uint8)
        st = np.zeros(n, np.int32)
        err = lib().fd_ed25519_gpu_debug_verify_dig(self._h, n, _p(blob), blob.nbytes, _p(desc), _p(dig), _p(codes), _p(k), _p(st))
        if err:
            raise EngineError(f"debug_verify_dig: {strerror(err)}: {last_error()}")
        return codes, k, st

    def debug_stages(self, blob: np.ndarray, desc: np.ndarray, dig=None) -> "Stages":
        """Diagnostics (fd_ed25519_gpu_debug_stages): one verify launch on the schedule
        the engine's mode and knobs give a batch of n, with the stages it leaves in the
        HBM working set read back.  dig None: the product's front end (real SHA-512);
        dig [n,64] uint8: the chosen-digest front end of debug_verify_dig.  Returns a
        Stages: codes[n], status[n] (prep's), pstat[2n], pts[2n,40] (A rows, then R
        rows), op_start[n], ops[n,512], tab[n,8,4,12] or None, fin[n,40] or None (pooled
        schedule only), schedule ("uniform", "pooled", "quad", "oct") and ops_sigmajor
        (the layout the device used; ops is delivered signature-major either way)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        n = len(desc)
        if dig is not None:
            dig = np.ascontiguousarray(dig, dtype=np.uint8)
            if dig.size != 64 * n:
                raise EngineError(f"debug_stages: dig holds {dig.size} bytes, not 64 per signature ({64 * n})")
        s = Stages()
        s.codes = np.zeros(n, np.int32)
        s.status = np.zeros(n, np.int32)
        s.pstat = np.zeros(2 * n, np.int32)
        s.pts = np.zeros((2 * n, 40), np.int32)
        s.op_start = np.zeros(n, np.int32)
        s.ops = np.zeros((n, 512), np.uint8)
        s.tab = np.zeros((n, 8, 4, 12), np.int32)
        s.fin = np.zeros((n, 40), np.int32)
        info = np.zeros(4, np.int32)
        err = lib().fd_ed25519_gpu_debug_stages(self._h, n, _p(blob), blob.nbytes, _p(desc), _p(dig) if dig is not None and n else None,
                                                _p(s.codes), _p(s.status), _p(s.pstat), _p(s.pts), _p(s.op_start), _p(s.ops),
                                                _p(s.tab), _p(s.fin), _p(info))
        if err:
            raise EngineError(f"debug_stages: {strerror(err)}: {last_error()}")
        s.schedule = ("uniform", "pooled", "quad", "oct")[int(info[0])]
        s.ops_sigmajor = bool(info[1])
        if not info[2]:
            s.tab = None
        if not info[3]:
            s.fin = None
        return s

    def debug_fe(self, op: int, f: np.ndarray, g: np.ndarray) -> np.ndarray:
        """Diagnostics: the device field products (fd_k_debug_fe op 0-6, op 7 the oct DSM's half product) of
        operand pairs f, g ([n,10] int32 limbs) -> [3,n,10] int32 limbs."""
        f = np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 10)
        g = np.ascontiguousarray(g, dtype=np.int32).reshape(-1, 10)
        if f.shape != g.shape:
            raise EngineError("debug_fe: f and g differ in shape")
        h = np.zeros((3, len(f), 10), np.int32)
        err = lib().fd_ed25519_gpu_debug_fe(self._h, int(op), len(f), _p(f), _p(g), _p(h))
        if err:
            raise EngineError(f"debug_fe: {strerror(err)}: {last_error()}")
        return h

    def sign_packed(self, blob: np.ndarray, sdesc: np.ndarray, want_pub: bool = True):
        """Sign a packed batch (fd_ed25519_gpu_sign_packed): sdesc is SIGN_DESC_DTYPE
        (seed_off, pub_off or SIGN_DERIVE, msg_off, msg_sz) -> (sig[n,64], pub[n,32] or
        None, codes[n]); an out-of-bounds entry gets ERR_ARG and zero bytes."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        sdesc = np.ascontiguousarray(sdesc, dtype=SIGN_DESC_DTYPE)
        n = len(sdesc)
        sig = np.zeros((n, 64), np.uint8)
        pub = np.zeros((n, 32), np.uint8) if want_pub else None
        codes = np.zeros(n, np.int32)
        err = lib().fd_ed25519_gpu_sign_packed(self._h, n, _p(blob), blob.nbytes, _p(sdesc), _p(sig),
                                               _p(pub) if want_pub else None, _p(codes))
        if err:
            raise EngineError(f"sign_packed: {strerror(err)}: {last_error()}")
        return sig, pub, codes

    def public_from_seeds(self, seeds: np.ndarray) -> np.ndarray:
        """Public keys [n,32] of seeds [n,32], derived on the device."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
        pub = np.zeros((len(seeds), 32), np.uint8)
        err = lib().fd_ed25519_gpu_public_packed(self._h, len(seeds), _p(seeds), _p(pub))
        if err:
            raise EngineError(f"public_from_seeds: {strerror(err)}: {last_error()}")
        return pub

    def sign_dev(self, n: int, d_blob: int, blob_sz: int, d_sdesc: int, d_sig_out: int, d_pub_out: int, d_out: int,
                 stream: int = 0) -> None:
        """Device-resident signing (raw device pointers; d_pub_out may be 0), ordered on
        `stream` as verify_dev.  The caller's memory: seeds in d_blob are not cleared."""
        err = lib().fd_ed25519_gpu_sign_dev(self._h, n, d_blob, blob_sz, d_sdesc, d_sig_out, d_pub_out or None, d_out,
                                            stream or None)
        if err:
            raise EngineError(f"sign_dev: {strerror(err)}: {last_error()}")

    def debug_sign_op(self, op: int, in0: np.ndarray, in1: np.ndarray = None, in2: np.ndarray = None) -> np.ndarray:
        """Diagnostics (fd_ed25519_gpu_debug_sign_op): op 0, the encodings of [s]B for
        scalars in0 [n,32]; op 1, (k a + r) mod L for k = in0, a = in1, r = in2 -> [n,32]."""
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 32) for x in (in0, in1, in2)]
        n = len(a[0])
        if any(x is not None and len(x) != n for x in a):
            raise EngineError("debug_sign_op: operands differ in length")
        out = np.zeros((n, 32), np.uint8)
        err = lib().fd_ed25519_gpu_debug_sign_op(self._h, int(op), n, *[None if x is None else _p(x) for x in a], _p(out))
        if err:
            raise EngineError(f"debug_sign_op: {strerror(err)}: {last_error()}")
        return out

    def txns_reserve(self, max_txn: int) -> None:
        """Allocate the scratch of the transaction calls for batches of up to max_txn
        transactions now (fd_ed25519_gpu_txns_reserve) instead of in the first call."""
        err = lib().fd_ed25519_gpu_txns_reserve(self._h, int(max_txn))
        if err:
            raise EngineError(f"txns_reserve: {strerror(err)}: {last_error()}")

    def verify_txns(self, blob: np.ndarray, txns: np.ndarray, want_codes: bool = False, txn_out_stride: int = 0):
        """Whole transactions, host buffers (fd_ed25519_gpu_verify_txns_packed): txns is
        TXN_DTYPE (payload t = blob[off, off+sz)) -> results (TXN_RESULT_DTYPE: status,
        sig_base, tag, footprint, reject_line, sig_cnt, version), or the tuple (results,
        codes, txn_out) when want_codes or txn_out_stride ask for more: codes the
        per-signature codes at sig_base + i (else None), txn_out [n, stride] uint8 with
        transaction t's fd_txn_t where 0 < footprint <= stride (zeros elsewhere; else None)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        n = len(txns)
        res = np.zeros(n, TXN_RESULT_DTYPE)
        codes = np.zeros(127 * n, np.int32) if want_codes else None
        out = np.zeros((n, txn_out_stride), np.uint8) if txn_out_stride else None
        err = lib().fd_ed25519_gpu_verify_txns_packed(self._h, n, _p(blob), blob.nbytes, _p(txns), _p(res),
                                                      _p(codes) if want_codes else None,
                                                      _p(out) if txn_out_stride else None, txn_out_stride)
        if err:
            raise EngineError(f"verify_txns: {strerror(err)}: {last_error()}")
        if not want_codes and not txn_out_stride:
            return res
        if want_codes:
            got = res["sig_cnt"] > 0
            n_sig = int((res["sig_base"][got].astype(np.int64) + res["sig_cnt"][got]).max()) if got.any() else 0
            codes = codes[:n_sig].copy()
        return res, codes, out

    def verify_txns_dev(self, n_txn: int, d_blob: int, blob_sz: int, d_txn: int, sig_cap: int, d_res: int,
                        d_codes: int = 0, d_txn_out: int = 0, txn_out_stride: int = 0, stream: int = 0,
                        timed: bool = False):
        """Device-resident transactions (fd_ed25519_gpu_verify_txns_dev; raw device
        pointers, d_codes and d_txn_out may be 0), ordered on `stream` as verify_dev.
        timed: block and return the four new kernels' durations (ms: parse, scan,
        expand, reduce)."""
        if timed:
            ms = np.zeros(4, np.float32)
            err = lib().fd_ed25519_gpu_verify_txns_dev_timed(self._h, n_txn, d_blob, blob_sz, d_txn, sig_cap, d_res, d_codes or None,
                                                             d_txn_out or None, txn_out_stride, stream or None, _p(ms))
        else:
            ms = None
            err = lib().fd_ed25519_gpu_verify_txns_dev(self._h, n_txn, d_blob, blob_sz, d_txn, sig_cap, d_res, d_codes or None,
                                                       d_txn_out or None, txn_out_stride, stream or None)
        if err:
            raise EngineError(f"verify_txns_dev: {strerror(err)}: {last_error()}")
        return ms

    def try_submit_txns(self, blob: np.ndarray, txns: np.ndarray):
        """Queue a batch of whole transactions on the pinned ring
        (fd_ed25519_gpu_try_submit_txns) -> its ticket, or None when the ring is full."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        t = ctypes.c_ulong(0)
        r = lib().fd_ed25519_gpu_try_submit_txns(self._h, len(txns), _p(blob), blob.nbytes, _p(txns), ctypes.byref(t))
        if r < 0:
            raise EngineError(f"try_submit_txns: {strerror(r)}: {last_error()}")
        if r == 0:
            return None
        self._pending_txns[t.value] = int(lib().fd_ed25519_gpu_txn_claims(_p(blob), blob.nbytes, _p(txns), len(txns), None))
        return t.value

    def submit_txns(self, blob: np.ndarray, txns: np.ndarray) -> int:
        """try_submit_txns, raising on a full ring as submit does."""
        t = self.try_submit_txns(blob, txns)
        if t is None:
            raise EngineError(f"submit_txns: {strerror(ERR_ARG)}: the ring is full")
        return t

    def poll_txns(self, ticket: int, n_txn: int, want_codes: bool = False, block: bool = True):
        """Collect a transaction ticket (fd_ed25519_gpu_poll_txns) -> its n_txn results
        (TXN_RESULT_DTYPE; sig_base is the prefix of the claims, txn_claims), or
        (results, codes) with the per-signature codes by claimed slot when want_codes;
        None while the batch is in flight (block=False)."""
        n_sig = self._pending_txns.get(ticket)
        if n_sig is None:
            raise EngineError(f"poll_txns: unknown ticket {ticket}")
        res = np.zeros(int(n_txn), TXN_RESULT_DTYPE)
        codes = np.zeros(max(n_sig, 1), np.int32) if want_codes else None
        r = lib().fd_ed25519_gpu_poll_txns(self._h, ticket, _p(res), _p(codes) if want_codes else None, 1 if block else 0)
        if r < 0:
            raise EngineError(f"poll_txns: {strerror(r)}: {last_error()}")
        if r == 0:
            return None
        del self._pending_txns[ticket]
        return (res, codes[:n_sig]) if want_codes else res

    def txn_ring_allocs(self) -> int:
        """Diagnostics: ring slots whose transaction scratch has been allocated."""
        return int(lib().fd_ed25519_gpu_txn_ring_allocs(self._h))

    TXN_RING_KERNELS = ("fd_k_txn_ring_front", "fd_k_txn_ring_reduce")

    def txn_ring_timed(self, blob: np.ndarray, txns: np.ndarray):
        """Diagnostics (fd_ed25519_gpu_txn_ring_timed): one ring batch, submitted and
        polled -> (results, the two ring kernels' durations in ms, TXN_RING_KERNELS order)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        res = np.zeros(len(txns), TXN_RESULT_DTYPE)
        ms = np.zeros(2, np.float32)
        err = lib().fd_ed25519_gpu_txn_ring_timed(self._h, len(txns), _p(blob), blob.nbytes, _p(txns), _p(res), _p(ms))
        if err:
            raise EngineError(f"txn_ring_timed: {strerror(err)}: {last_error()}")
        return res, ms

    TXN_KERNELS = ("fd_k_txn_parse", "fd_k_txn_scan", "fd_k_txn_expand", "fd_k_txn_reduce")

    def debug_txn_descs(self, blob: np.ndarray, txns: np.ndarray, sig_cap: int):
        """Diagnostics (fd_ed25519_gpu_debug_txn_descs): parse, scan and expand only ->
        (desc[sig_cap] as fd_k_txn_expand wrote every slot, n_sig, results)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
        desc = np.zeros(sig_cap, DESC_DTYPE)
        res = np.zeros(len(txns), TXN_RESULT_DTYPE)
        n_sig = ctypes.c_ulong(0)
        err = lib().fd_ed25519_gpu_debug_txn_descs(self._h, len(txns), _p(blob), blob.nbytes, _p(txns), sig_cap, _p(desc),
                                                   ctypes.byref(n_sig), _p(res))
        if err:
            raise EngineError(f"debug_txn_descs: {strerror(err)}: {last_error()}")
        return desc, n_sig.value, res

    def poh_verify(self, entries: np.ndarray, n_max: int, states: bool = False):
        """fd_poh_gpu_verify_packed: the code of every Proof-of-History entry
        (0, POH_ERR_HASH, ERR_ARG for an entry the header refuses), lanes
        ordered by n descending on the device.  states: also each entry's
        final 32-byte state, as an (n, 32) array."""
        entries = np.ascontiguousarray(entries, dtype=POH_ENTRY_DTYPE)
        n = len(entries)
        out = np.empty(n, dtype=np.int32)
        st = np.empty((n, 32), dtype=np.uint8) if states else None
        err = lib().fd_poh_gpu_verify_packed(self._h, n, _p(entries), n_max, _p(out), _p(st) if states else None)
        if err:
            raise EngineError(f"poh_verify: {strerror(err)}: {last_error()}")
        return (out, st) if states else out

    def poh_verify_dev(self, n: int, d_entries: int, n_max: int, d_out: int, d_states: int = 0, d_work: int = 0,
                       stream: int = 0) -> None:
        """fd_poh_gpu_verify_dev: device-resident entries in the caller's lane
        order (raw device pointers; d_work: poh_work_sz(n) bytes); queues the
        launches and returns."""
        err = lib().fd_poh_gpu_verify_dev(self._h, n, d_entries, n_max, d_out, d_states or None, d_work or None, stream or None)
        if err:
            raise EngineError(f"poh_verify_dev: {strerror(err)}: {last_error()}")

    @property
    def poh_chunk(self) -> int:
        """hashes one lane runs per launch (fd_poh_gpu_debug_set_chunk; 0 sets the default)"""
        return lib().fd_poh_gpu_chunk(self._h)

    @poh_chunk.setter
    def poh_chunk(self, c: int) -> None:
        if lib().fd_poh_gpu_debug_set_chunk(self._h, c):
            raise EngineError(f"poh_chunk: bad chunk {c}")

    def poh_debug_sort(self, on: bool) -> None:
        """experiments: False keeps the caller's lane order in poh_verify"""
        if lib().fd_poh_gpu_debug_set_sort(self._h, 1 if on else 0):
            raise EngineError(f"poh_debug_sort: {last_error()}")

    def poh_verify_entries(self, entries: np.ndarray, n_max: int, leaf_cnt: np.ndarray, leaves: np.ndarray, blob: np.ndarray,
                           leaf_max: int, states: bool = False):
        """fd_poh_gpu_verify_entries_packed: poh_verify where entry i with
        leaf_cnt[i] > 0 takes its mixin from the bmtree32 root of its leaves
        (BMTREE_LEAF_DTYPE descriptors into blob), computed on the device."""
        entries = np.ascontiguousarray(entries, dtype=POH_ENTRY_DTYPE)
        leaf_cnt, leaves, blob = _bmtree_inputs(leaf_cnt, leaves, blob)
        n = len(entries)
        if len(leaf_cnt) != n:
            raise ValueError("poh_verify_entries: one leaf count per entry")
        out = np.empty(n, dtype=np.int32)
        st = np.empty((n, 32), dtype=np.uint8) if states else None
        err = lib().fd_poh_gpu_verify_entries_packed(self._h, n, _p(entries), n_max, _p(out), _p(st) if states else None,
                                                     _p(leaf_cnt), _p(leaves), _p(blob), blob.nbytes, leaf_max)
        if err:
            raise EngineError(f"poh_verify_entries: {strerror(err)}: {last_error()}")
        return (out, st) if states else out

    def poh_verify_entries_dev(self, n: int, d_entries: int, n_max: int, d_out: int, d_states: int, d_work: int, d_first: int,
                               n_leaves: int, d_leaves: int, d_blob: int, blob_sz: int, leaf_max: int, d_tree_work: int,
                               stream: int = 0) -> None:
        """fd_poh_gpu_verify_entries_dev (raw device pointers; d_tree_work:
        poh_entries_work_sz(n, n_leaves) bytes); queues the launches and
        returns.  The entries are written (mixin, _pad)."""
        err = lib().fd_poh_gpu_verify_entries_dev(self._h, n, d_entries, n_max, d_out, d_states or None, d_work or None,
                                                  d_first or None, n_leaves, d_leaves or None, d_blob or None, blob_sz, leaf_max,
                                                  d_tree_work or None, stream or None)
        if err:
            raise EngineError(f"poh_verify_entries_dev: {strerror(err)}: {last_error()}")

    def bmtree_roots(self, width: int, leaf_cnt: np.ndarray, leaves: np.ndarray, blob: np.ndarray, leaf_max: int, flags: int = 0):
        """fd_bmtree_gpu_roots_packed: the Merkle root of every tree as an
        (n_trees, 32) array (width 20: bytes 20..31 zero) and its code (0, or
        ERR_ARG for a refused tree, whose root is zero)."""
        leaf_cnt, leaves, blob = _bmtree_inputs(leaf_cnt, leaves, blob)
        n = len(leaf_cnt)
        roots = np.empty((n, 32), dtype=np.uint8)
        codes = np.empty(n, dtype=np.int32)
        err = lib().fd_bmtree_gpu_roots_packed(self._h, width, flags, n, _p(leaf_cnt), _p(leaves), _p(blob), blob.nbytes, leaf_max,
                                               _p(roots), _p(codes))
        if err:
            raise EngineError(f"bmtree_roots: {strerror(err)}: {last_error()}")
        return roots, codes

    def bmtree_roots_dev(self, width: int, n_trees: int, d_first: int, n_leaves: int, d_leaves: int, d_blob: int, blob_sz: int,
                         leaf_max: int, d_roots: int, root_stride: int, d_codes: int, d_work: int, stream: int = 0,
                         flags: int = 0) -> None:
        """fd_bmtree_gpu_roots_dev: device-resident (raw device pointers;
        d_work: bmtree_work_sz(n_trees, n_leaves) bytes); queues the launches
        and returns."""
        err = lib().fd_bmtree_gpu_roots_dev(self._h, width, flags, n_trees, d_first or None, n_leaves, d_leaves or None,
                                            d_blob or None, blob_sz, leaf_max, d_roots or None, root_stride, d_codes or None,
                                            d_work or None, stream or None)
        if err:
            raise EngineError(f"bmtree_roots_dev: {strerror(err)}: {last_error()}")

    def bmtree_proofs(self, width: int, leaf_cnt: np.ndarray, leaves: np.ndarray, blob: np.ndarray, leaf_max: int, flags: int = 0,
                      proofs: np.ndarray = None):
        """fd_bmtree_gpu_proofs_packed: bmtree_roots, and every leaf's
        inclusion proof.  proofs: a C-contiguous (n_leaves, stride) uint8
        array that receives leaf k's proof in row k, every other byte left
        as it is (default: zeros of the smallest stride).  Returns (roots,
        codes, proofs)."""
        leaf_cnt, leaves, blob = _bmtree_inputs(leaf_cnt, leaves, blob)
        n = len(leaf_cnt)
        proofs = _bmtree_proof_rows(width, len(leaves), leaf_max, proofs)
        roots = np.empty((n, 32), dtype=np.uint8)
        codes = np.empty(n, dtype=np.int32)
        err = lib().fd_bmtree_gpu_proofs_packed(self._h, width, flags, n, _p(leaf_cnt), _p(leaves), _p(blob), blob.nbytes, leaf_max,
                                                _p(roots), _p(codes), _p(proofs), proofs.shape[1])
        if err:
            raise EngineError(f"bmtree_proofs: {strerror(err)}: {last_error()}")
        return roots, codes, proofs

    def bmtree_proofs_dev(self, width: int, n_trees: int, d_first: int, n_leaves: int, d_leaves: int, d_blob: int, blob_sz: int,
                          leaf_max: int, d_roots: int, root_stride: int, d_proofs: int, proof_stride: int, d_codes: int, d_work: int,
                          stream: int = 0, flags: int = 0) -> None:
        """fd_bmtree_gpu_proofs_dev: bmtree_roots_dev, and leaf k's proof to
        d_proofs + k proof_stride; queues the launches and returns."""
        err = lib().fd_bmtree_gpu_proofs_dev(self._h, width, flags, n_trees, d_first or None, n_leaves, d_leaves or None,
                                             d_blob or None, blob_sz, leaf_max, d_roots or None, root_stride, d_proofs or None,
                                             proof_stride, d_codes or None, d_work or None, stream or None)
        if err:
            raise EngineError(f"bmtree_proofs_dev: {strerror(err)}: {last_error()}")

    def bmtree_from_proofs(self, width: int, proofs: np.ndarray, blob: np.ndarray, depth_max: int, flags: int = 0):
        """fd_bmtree_gpu_from_proofs_packed: the root every leaf and proof
        (BMTREE_PROOF_DTYPE descriptors into blob) lead to as an (n, 32)
        array, and its code (0, BMTREE_ERR_PROOF, or ERR_ARG for a refused
        descriptor, whose root is zero)."""
        proofs = np.ascontiguousarray(proofs, dtype=BMTREE_PROOF_DTYPE)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        n = len(proofs)
        roots = np.empty((n, 32), dtype=np.uint8)
        codes = np.empty(n, dtype=np.int32)
        err = lib().fd_bmtree_gpu_from_proofs_packed(self._h, width, flags, n, _p(proofs), _p(blob), blob.nbytes, depth_max,
                                                     _p(roots), _p(codes))
        if err:
            raise EngineError(f"bmtree_from_proofs: {strerror(err)}: {last_error()}")
        return roots, codes

    def bmtree_from_proofs_dev(self, width: int, n: int, d_proofs: int, d_blob: int, blob_sz: int, depth_max: int, d_roots: int,
                               root_stride: int, d_codes: int, stream: int = 0, flags: int = 0) -> None:
        """fd_bmtree_gpu_from_proofs_dev: device-resident (raw device
        pointers); queues one launch and returns."""
        err = lib().fd_bmtree_gpu_from_proofs_dev(self._h, width, flags, n, d_proofs or None, d_blob or None, blob_sz, depth_max,
                                                  d_roots or None, root_stride, d_codes or None, stream or None)
        if err:
            raise EngineError(f"bmtree_from_proofs_dev: {strerror(err)}: {last_error()}")

    def sha512(self, msgs, is384: bool = False) -> list:
        """SHA-512 (SHA-384) digests of byte strings on the device."""
        n = len(msgs)
        if n == 0:
            return []
        offs, parts, o = [], [], 0
        for m in msgs:
            offs.append(o)
            parts.append(bytes(m) + b"\0" * ((-len(m)) % 8))
            o += len(parts[-1])
        blob = np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()
        desc = np.zeros(n, DESC_DTYPE)
        desc["msg_off"] = offs
        desc["msg_sz"] = [len(m) for m in msgs]
        hsz = 48 if is384 else 64
        out = np.zeros(n * hsz, np.uint8)
        err = lib().fd_ed25519_gpu_sha512_packed(self._h, n, _p(blob), o, _p(desc), _p(out), 1 if is384 else 0)
        if err:
            raise EngineError(f"sha512_packed: {strerror(err)}: {last_error()}")
        return [out[i * hsz:(i + 1) * hsz].tobytes() for i in range(n)]

    def sha512_any(self, msgs, is384: bool = False) -> list:
        """fd_ed25519_gpu_sha512_ptrs: SHA-512 (SHA-384) digests of byte
        strings of any length (past max_blob: the long path)."""
        return _sha512_ptrs(self._h, msgs, is384)

    @property
    def mode(self) -> int:
        return lib().fd_ed25519_gpu_mode(self._h)

    @mode.setter
    def mode(self, m: int) -> None:
        if lib().fd_ed25519_gpu_set_mode(self._h, m):
            raise EngineError(f"bad mode {m}")

    @property
    def dsm_pool_min(self) -> int:
        """batches of at least this many signatures take the pooled DSM"""
        return lib().fd_ed25519_gpu_dsm_pool_min(self._h)

    @dsm_pool_min.setter
    def dsm_pool_min(self, n: int) -> None:
        if lib().fd_ed25519_gpu_set_dsm_pool_min(self._h, n):
            raise EngineError("set_dsm_pool_min")

    @property
    def dsm_quad_max(self) -> int:
        """smaller batches of at most this many signatures take the quad-lane DSM"""
        return lib().fd_ed25519_gpu_dsm_quad_max(self._h)

    @dsm_quad_max.setter
    def dsm_quad_max(self, n: int) -> None:
        if lib().fd_ed25519_gpu_set_dsm_quad_max(self._h, n):
            raise EngineError("set_dsm_quad_max")

    @property
    def dsm_oct_max(self) -> int:
        """batches of at most this many signatures (below dsm_pool_min) run the eight-lane DSM"""
        return lib().fd_ed25519_gpu_dsm_oct_max(self._h)

    @dsm_oct_max.setter
    def dsm_oct_max(self, n: int) -> None:
        if lib().fd_ed25519_gpu_set_dsm_oct_max(self._h, n):
            raise EngineError("set_dsm_oct_max")

    @property
    def depth(self) -> int:
        return lib().fd_ed25519_gpu_depth(self._h)

    @property
    def cu_groups(self) -> int:
        """CU groups the ring's small batches are spread over (1: none)"""
        return lib().fd_ed25519_gpu_cu_groups(self._h)

    @cu_groups.setter
    def cu_groups(self, g: int) -> None:
        if lib().fd_ed25519_gpu_set_cu_groups(self._h, int(g)):
            raise EngineError(f"set_cu_groups({g}): ring busy or bad count")

    def register(self, host: np.ndarray) -> None:
        """Let the ring DMA batches straight from this (contiguous) host array."""
        if not host.flags.c_contiguous:
            raise EngineError("register: array must be contiguous")
        if lib().fd_ed25519_gpu_register(self._h, _p(host), host.nbytes):
            raise EngineError(f"register: {last_error()}")
        self._registered.append(host)

    def unregister(self, host: np.ndarray) -> None:
        if lib().fd_ed25519_gpu_unregister(self._h, _p(host)):
            raise EngineError(f"unregister: {last_error()}")
        self._registered = [a for a in self._registered if a is not host]


class Job(ctypes.Structure):
    """fd_ed25519_gpu_job_t"""
    _fields_ = [("n", ctypes.c_ulong), ("blob", ctypes.c_void_p), ("blob_sz", ctypes.c_ulong),
                ("desc", ctypes.c_void_p), ("out", ctypes.c_void_p), ("state", ctypes.c_int),
                ("t_push_ns", ctypes.c_ulong), ("t_submit_ns", ctypes.c_ulong), ("t_done_ns", ctypes.c_ulong),
                ("t_pick_ns", ctypes.c_ulong), ("blob2", ctypes.c_void_p), ("blob2_sz", ctypes.c_ulong)]


# fd_ed25519_gpu_synth_stat_t
SYNTH_STAT_DTYPE = np.dtype([("t_sched_ns", "<u8"), ("t_push_ns", "<u8"), ("t_submit_ns", "<u8"), ("t_done_ns", "<u8"),
                             ("t_pick_ns", "<u8"), ("state", "<i4"), ("codes", "<u4", (5,))], align=True)


class Feeder:
    """The per-GPU feeder thread (fd_ed25519_gpu_feeder_t) over an Engine's ring."""

    def __init__(self, engine: Engine, pin_numa: bool = True):
        self.engine = engine
        self._h = lib().fd_ed25519_gpu_feeder_new(engine._h, 1 if pin_numa else 0)
        if not self._h:
            raise EngineError("fd_ed25519_gpu_feeder_new failed")
        self._keep = {}

    @property
    def numa_node(self) -> int:
        return lib().fd_ed25519_gpu_feeder_numa_node(self._h)

    def push(self, blob: np.ndarray, desc: np.ndarray, out: np.ndarray, job: Job = None) -> Job:
        """Queue a batch; the arrays must stay alive and unchanged until the job completes."""
        if blob.dtype != np.uint8 or not blob.flags.c_contiguous or desc.dtype != DESC_DTYPE or not desc.flags.c_contiguous:
            raise EngineError("push: contiguous uint8 blob and DESC_DTYPE desc required")
        if out.dtype != np.int32 or not out.flags.c_contiguous or out.size < len(desc):
            raise EngineError("push: out must be a contiguous int32 array of >= len(desc) entries")
        j = job if job is not None else Job()
        j.n, j.blob, j.blob_sz, j.desc, j.out = len(desc), blob.ctypes.data, blob.nbytes, desc.ctypes.data, out.ctypes.data
        self._keep[ctypes.addressof(j)] = (blob, desc, out)
        err = lib().fd_ed25519_gpu_feeder_push(self._h, ctypes.byref(j))
        if err:
            raise EngineError(f"feeder push: {strerror(err)}")
        return j

    def wait(self, job: Job, timeout_ns: int = -1) -> None:
        err = lib().fd_ed25519_gpu_job_wait(ctypes.byref(job), timeout_ns)
        # the arrays stay referenced until the job reached a final state: after
        # a timeout it is still queued or in flight on the feeder thread, which
        # may yet read the blob and descriptors and write the codes
        # (close() releases them once the feeder has drained)
        if job.state != 0:
            self._keep.pop(ctypes.addressof(job), None)
        if err:
            raise EngineError(f"job: {strerror(err)}: {last_error()}")

    def synth(self, blob: np.ndarray, desc: np.ndarray, batch_sigs: int, starts, nbatch: int, window: int,
              period_ns: int = 0, codes: bool = False):
        """The native synthetic-load producer (fd_ed25519_gpu_feeder_synth): nbatch
        jobs of batch_sigs signatures, job i from desc[starts[i % len(starts)]:],
        closed loop with `window` outstanding (period_ns 0) or paced one job per
        period_ns.  Returns the per-job SYNTH_STAT_DTYPE records, and with
        codes=True also every code as int8 [nbatch, batch_sigs]."""
        blob = np.ascontiguousarray(blob, np.uint8)
        desc = np.ascontiguousarray(desc, DESC_DTYPE)
        st = np.ascontiguousarray(starts, np.uint64)
        stat = np.zeros(nbatch, SYNTH_STAT_DTYPE)
        cs = np.full((nbatch, batch_sigs), 99, np.int8) if codes else None
        err = lib().fd_ed25519_gpu_feeder_synth(self._h, _p(blob), blob.nbytes, _p(desc), len(desc), batch_sigs,
                                                _p(st), len(st), nbatch, window, period_ns, _p(stat),
                                                _p(cs) if codes else None)
        if err:
            raise EngineError(f"feeder synth: {strerror(err)}: {last_error()}")
        return (stat, cs) if codes else stat

    def close(self):
        if self._h:
            lib().fd_ed25519_gpu_feeder_delete(self._h)
            self._h = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiEngine:
    """Engines on several devices (repeats allowed) behind one host:
    fd_ed25519_gpu_multi_t."""

    def __init__(self, devices, max_sigs: int = 1 << 16, max_blob: int = 1 << 26, depth: int = 3):
        d = np.ascontiguousarray(devices, np.int32)
        self._h = lib().fd_ed25519_gpu_multi_new_ex(_p(d), len(d), max_sigs, max_blob, depth)
        if not self._h:
            raise EngineError(f"fd_ed25519_gpu_multi_new({list(devices)}) failed: {last_error()}")

    def verify_packed(self, blob: np.ndarray, desc: np.ndarray) -> np.ndarray:
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=DESC_DTYPE)
        out = np.empty(len(desc), dtype=np.int32)
        err = lib().fd_ed25519_gpu_multi_verify_packed(self._h, len(desc), _p(blob), blob.nbytes, _p(desc), _p(out))
        if err:
            raise EngineError(f"multi verify_packed: {strerror(err)}: {last_error()}")
        return out

    @property
    def count(self) -> int:
        return lib().fd_ed25519_gpu_multi_cnt(self._h)

    def close(self):
        if self._h:
            lib().fd_ed25519_gpu_multi_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def codes_to_bitmap(codes: np.ndarray) -> np.ndarray:
    codes = np.ascontiguousarray(codes, np.int32)
    bm = np.zeros((len(codes) + 7) // 8, np.uint8)
    lib().fd_ed25519_codes_to_bitmap(len(codes), _p(codes), _p(bm))
    return bm


def verify(msg: bytes, sig: bytes, pub: bytes) -> int:
    """fd_ed25519_verify on the process-default engine."""
    m = ctypes.create_string_buffer(bytes(msg), max(1, len(msg)))
    s = ctypes.create_string_buffer(bytes(sig), 64)
    p = ctypes.create_string_buffer(bytes(pub), 32)
    return lib().fd_ed25519_verify(m, len(msg), s, p, None)


def verify_batch(msgs, sigs, pubs) -> tuple[int, np.ndarray]:
    """fd_ed25519_verify_batch over Python byte strings."""
    n = len(msgs)
    bufs = [ctypes.create_string_buffer(bytes(m), max(1, len(m))) for m in msgs]
    sb = [ctypes.create_string_buffer(bytes(s), 64) for s in sigs]
    pb = [ctypes.create_string_buffer(bytes(p), 32) for p in pubs]
    MP = ctypes.c_void_p * n
    mp = MP(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sp = MP(*[ctypes.cast(b, ctypes.c_void_p) for b in sb])
    pp = MP(*[ctypes.cast(b, ctypes.c_void_p) for b in pb])
    sz = (ctypes.c_ulong * n)(*[len(m) for m in msgs])
    out = np.zeros(n, dtype=np.int32)
    r = lib().fd_ed25519_verify_batch(n, mp, sz, sp, pp, _p(out))
    return r, out


def verify_batch_single_msg(msg: bytes, sigs: np.ndarray, pubs: np.ndarray) -> tuple[int, np.ndarray]:
    sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 64)
    pubs = np.ascontiguousarray(pubs, dtype=np.uint8).reshape(-1, 32)
    n = len(sigs)
    m = ctypes.create_string_buffer(bytes(msg), max(1, len(msg)))
    out = np.zeros(n, dtype=np.int32)
    r = lib().fd_ed25519_verify_batch_single_msg(m, len(msg), _p(sigs), _p(pubs), n, _p(out))
    return r, out


def _poh_state(state: bytes):
    """a 32-byte state in a 32-aligned buffer (fd_poh_state_t): (keepalive, address)"""
    if len(state) != 32:
        raise ValueError("a PoH state is 32 bytes")
    buf = ctypes.create_string_buffer(64)
    a = (ctypes.addressof(buf) + 31) & ~31
    ctypes.memmove(a, bytes(state), 32)
    return buf, a


def poh_append(state: bytes, n: int) -> bytes:
    """fd_poh_append on the host: n recursive SHA-256 hashes of a 32-byte state"""
    buf, a = _poh_state(state)
    lib().fd_poh_append(a, n)
    return ctypes.string_at(a, 32)


def poh_mixin(state: bytes, mixin: bytes) -> bytes:
    """fd_poh_mixin on the host: SHA-256( state || mixin )"""
    if len(mixin) != 32:
        raise ValueError("a PoH mixin is 32 bytes")
    buf, a = _poh_state(state)
    lib().fd_poh_mixin(a, bytes(mixin))
    return ctypes.string_at(a, 32)


def poh_verify_batch(entries: np.ndarray, n_max: int, states: bool = False, nthreads: int = 8):
    """fd_poh_verify_batch: Engine.poh_verify's semantics on host threads"""
    entries = np.ascontiguousarray(entries, dtype=POH_ENTRY_DTYPE)
    n = len(entries)
    out = np.empty(n, dtype=np.int32)
    st = np.empty((n, 32), dtype=np.uint8) if states else None
    err = lib().fd_poh_verify_batch(n, _p(entries), n_max, _p(out), _p(st) if states else None, nthreads)
    if err:
        raise EngineError(f"poh_verify_batch: {strerror(err)}")
    return (out, st) if states else out


def poh_chain(seed: bytes, hashes: np.ndarray, entries: np.ndarray) -> np.ndarray:
    """fd_poh_gpu_chain: fill start and expect of consecutive entries (in
    place) from the hash before the run and the (n, 32) hashes they claim"""
    hashes = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
    if entries.dtype != POH_ENTRY_DTYPE or not entries.flags.c_contiguous or len(entries) != len(hashes) or len(seed) != 32:
        raise ValueError("poh_chain: contiguous POH_ENTRY_DTYPE entries, one 32-byte hash each, a 32-byte seed")
    lib().fd_poh_gpu_chain(len(entries), bytes(seed), _p(hashes), _p(entries))
    return entries


def poh_work_sz(n: int) -> int:
    return lib().fd_poh_gpu_work_sz(n)


def poh_entries_work_sz(n: int, n_leaves: int) -> int:
    return lib().fd_poh_gpu_entries_work_sz(n, n_leaves)


def _bmtree_inputs(leaf_cnt, leaves, blob):
    leaf_cnt = np.ascontiguousarray(leaf_cnt, dtype=np.uint32)
    leaves = np.ascontiguousarray(leaves, dtype=BMTREE_LEAF_DTYPE)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if int(leaf_cnt.sum(dtype=np.uint64)) != len(leaves):
        raise ValueError("bmtree: the leaf counts do not sum to the number of descriptors")
    return leaf_cnt, leaves, blob


def _bmtree_node_buf(count: int):
    """count 32-byte nodes in a 32-aligned buffer: (keepalive, address)"""
    raw = np.zeros(32 * count + 32, dtype=np.uint8)
    a = (raw.ctypes.data + 31) & ~31
    return raw, a


def bmtree_hash_leaf(width: int, data: bytes) -> bytes:
    """fd_bmtree{20,32}_hash_leaf on the host: the first `width` bytes of SHA-256( 0x00 || data )"""
    raw, a = _bmtree_node_buf(1)
    data = bytes(data)
    getattr(lib(), f"fd_bmtree{width}_hash_leaf")(a, data, len(data))
    return ctypes.string_at(a, width)


class BmtreeCommit:
    """fd_bmtree{20,32}_commit_*: an incremental Merkle commitment on the host"""

    def __init__(self, width: int):
        if width not in (20, 32):
            raise ValueError("bmtree: width 20 or 32")
        self.width, L = width, lib()
        self._f = {k: getattr(L, f"fd_bmtree{width}_commit_{k}") for k in ("align", "footprint", "init", "leaf_cnt", "append", "fini")}
        al, fp = self._f["align"](), self._f["footprint"]()
        self._raw = np.zeros(fp + al, dtype=np.uint8)
        self._mem = (self._raw.ctypes.data + al - 1) & ~(al - 1)
        if self._f["init"](self._mem) != self._mem:
            raise EngineError("bmtree commit_init")

    @property
    def leaf_cnt(self) -> int:
        return self._f["leaf_cnt"](self._mem)

    def append(self, nodes) -> "BmtreeCommit":
        """nodes: byte strings of `width` (or 32) bytes each, in order"""
        raw, a = _bmtree_node_buf(len(nodes))
        for i, nd in enumerate(nodes):
            ctypes.memmove(a + 32 * i, bytes(nd), len(nd))
        self._f["append"](self._mem, a, len(nodes))
        return self

    def fini(self) -> bytes:
        return ctypes.string_at(self._f["fini"](self._mem), self.width)


def bmtree_roots_batch(width: int, leaf_cnt, leaves, blob, leaf_max: int, flags: int = 0, nthreads: int = 8):
    """fd_bmtree_roots_batch: Engine.bmtree_roots's semantics on host threads"""
    leaf_cnt, leaves, blob = _bmtree_inputs(leaf_cnt, leaves, blob)
    n = len(leaf_cnt)
    roots = np.empty((n, 32), dtype=np.uint8)
    codes = np.empty(n, dtype=np.int32)
    err = lib().fd_bmtree_roots_batch(width, flags, n, _p(leaf_cnt), _p(leaves), _p(blob), blob.nbytes, leaf_max, _p(roots), _p(codes),
                                      nthreads)
    if err:
        raise EngineError(f"bmtree_roots_batch: {strerror(err)}")
    return roots, codes


def bmtree_proof_stride(width: int, n_leaves: int, leaf_max: int) -> int:
    """the smallest proof_stride of an emit call: width * ceil_log2(min(leaf_max, n_leaves))"""
    m = min(int(leaf_max), int(n_leaves))
    return width * (m - 1).bit_length() if m > 1 else 0


def _bmtree_proof_rows(width: int, n_leaves: int, leaf_max: int, proofs):
    if proofs is None:
        return np.zeros((n_leaves, max(bmtree_proof_stride(width, n_leaves, leaf_max), 4)), dtype=np.uint8)
    if proofs.dtype != np.uint8 or proofs.ndim != 2 or len(proofs) != n_leaves or not proofs.flags.c_contiguous:
        raise ValueError("bmtree: proofs is a C-contiguous (n_leaves, stride) uint8 array")
    return proofs


def bmtree_proofs_batch(width: int, leaf_cnt, leaves, blob, leaf_max: int, flags: int = 0, nthreads: int = 8, proofs=None):
    """fd_bmtree_proofs_batch: Engine.bmtree_proofs's semantics on host threads"""
    leaf_cnt, leaves, blob = _bmtree_inputs(leaf_cnt, leaves, blob)
    n = len(leaf_cnt)
    proofs = _bmtree_proof_rows(width, len(leaves), leaf_max, proofs)
    roots = np.empty((n, 32), dtype=np.uint8)
    codes = np.empty(n, dtype=np.int32)
    err = lib().fd_bmtree_proofs_batch(width, flags, n, _p(leaf_cnt), _p(leaves), _p(blob), blob.nbytes, leaf_max, _p(roots), _p(codes),
                                       _p(proofs), proofs.shape[1], nthreads)
    if err:
        raise EngineError(f"bmtree_proofs_batch: {strerror(err)}")
    return roots, codes, proofs


def bmtree_from_proofs_batch(width: int, proofs, blob, depth_max: int, flags: int = 0, nthreads: int = 8):
    """fd_bmtree_from_proofs_batch: Engine.bmtree_from_proofs's semantics on host threads"""
    proofs = np.ascontiguousarray(proofs, dtype=BMTREE_PROOF_DTYPE)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = len(proofs)
    roots = np.empty((n, 32), dtype=np.uint8)
    codes = np.empty(n, dtype=np.int32)
    err = lib().fd_bmtree_from_proofs_batch(width, flags, n, _p(proofs), _p(blob), blob.nbytes, depth_max, _p(roots), _p(codes), nthreads)
    if err:
        raise EngineError(f"bmtree_from_proofs_batch: {strerror(err)}")
    return roots, codes


def bmtree_work_sz(n_trees: int, n_leaves: int) -> int:
    return lib().fd_bmtree_gpu_work_sz(n_trees, n_leaves)


def bmtree_merge_passes(width: int, leaf_cnt) -> int:
    """64-lane compression passes the merge launches issue for these tree sizes"""
    leaf_cnt = np.ascontiguousarray(leaf_cnt, dtype=np.uint32)
    return lib().fd_bmtree_gpu_merge_passes(width, len(leaf_cnt), _p(leaf_cnt))


def txn_claims(blob: np.ndarray, txns: np.ndarray):
    """fd_ed25519_gpu_txn_claims -> (bases[n_txn + 1] uint32, n_sig): the slots a ring
    batch's transactions claim by their first payload byte, as an exclusive prefix."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    txns = np.ascontiguousarray(txns, dtype=TXN_DTYPE)
    bases = np.zeros(len(txns) + 1, np.uint32)
    n_sig = lib().fd_ed25519_gpu_txn_claims(_p(blob), blob.nbytes, _p(txns), len(txns), _p(bases))
    return bases, int(n_sig)


def device_count() -> int:
    return lib().fd_ed25519_gpu_device_cnt()


def kernels_id() -> str:
    """build id of the loaded library's device code (fd_ed25519_gpu_kernels_id)"""
    f = lib().fd_ed25519_gpu_kernels_id
    f.restype = ctypes.c_char_p
    return f().decode()


def numa_cpus(device: int) -> list:
    """CPUs of the device's NUMA node this process may use ([] if unknown)."""
    node = lib().fd_ed25519_gpu_device_numa_node(device)
    if node < 0:
        return []
    cpus = set()
    for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return sorted(cpus & os.sched_getaffinity(0))


def _cpu_times() -> dict:
    out = {}
    for line in open("/proc/stat"):
        if line.startswith("cpu") and line[3].isdigit():
            f = line.split()
            v = [int(x) for x in f[1:]]
            out[int(f[0][3:])] = (v[3] + (v[4] if len(v) > 4 else 0), sum(v))   # (idle + iowait, total)
    return out


def _core_siblings(c: int) -> set:
    try:
        txt = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
    except OSError:
        return {c}
    sib = set()
    for part in txt.split(","):
        lo, _, hi = part.partition("-")
        sib.update(range(int(lo), int(hi or lo) + 1))
    return sib


def _l3_group(c: int) -> str:
    try:
        return open(f"/sys/devices/system/cpu/cpu{c}/cache/index3/shared_cpu_list").read().strip()
    except OSError:
        return ""


def quiet_cpus(n: int, device: int = 0, sample_s: float = 0.3, pairs: bool = True) -> list:
    """n CPUs for spinning host threads (tiles, feeders, producers): on the
    device's NUMA node, not CPU 0, one per physical core, the least busy over
    a short /proc/stat sample counting each core's other hardware threads --
    on a shared host other work lands on some CPUs, and a spinning thread
    that shares its core with it stalls for milliseconds.  pairs: CPUs
    2k and 2k+1 (a producer and its consumer) share a last-level cache, so
    the bytes one writes reach the other without crossing chiplets (on the
    GPU box's EPYC one CCD of 8 cores per L3).  [] if that many cannot be
    found."""
    import time
    cand = [c for c in (numa_cpus(device) or sorted(os.sched_getaffinity(0))) if c != 0]
    if len(cand) < n:
        return []
    t0 = _cpu_times()
    time.sleep(sample_s)
    t1 = _cpu_times()

    def busy(c):
        if c not in t0 or c not in t1 or t1[c][1] <= t0[c][1]:
            return 0.0
        return 1.0 - (t1[c][0] - t0[c][0]) / (t1[c][1] - t0[c][1])
    score = {c: sum(busy(x) for x in _core_siblings(c)) for c in cand}
    order = sorted(cand, key=lambda c: (score[c], c))
    pick, used = [], set()
    if pairs and n >= 2:
        # quietest pairs first, each pair from one L3 group
        while len(pick) + 2 <= n:
            best = None
            groups = {}
            for c in order:
                if c in used:
                    continue
                groups.setdefault(_l3_group(c), []).append(c)
            for g, cs in groups.items():
                two = []
                seen = set()
                for c in cs:                          # one per physical core
                    if c in seen:
                        continue
                    two.append(c)
                    seen |= _core_siblings(c)
                    if len(two) == 2:
                        break
                if len(two) == 2 and (best is None or score[two[0]] + score[two[1]] < best[0]):
                    best = (score[two[0]] + score[two[1]], two)
            if best is None:
                break
            for c in best[1]:
                pick.append(c)
                used |= _core_siblings(c)
        if len(pick) == n:
            return pick
        if len(pick) + 1 != n:
            pick, used = [], set()
    for c in order:
        if c in used:
            continue
        pick.append(c)
        used |= _core_siblings(c)
        if len(pick) == n:
            return pick
    return []


def sign_batch(seeds: np.ndarray, blob: np.ndarray, msg_off: np.ndarray, msg_sz: np.ndarray, nthreads: int = 8):
    """Host signer (test-data generation only): returns (pub[n,32], sig[n,64])."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
    n = len(seeds)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64)
    msg_sz = np.ascontiguousarray(msg_sz, dtype=np.uint32)
    pub = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    lib().fd_ed25519_sign_batch(n, _p(seeds), _p(blob), _p(msg_off), _p(msg_sz), _p(pub), _p(sig), nthreads)
    return pub, sig


def sign_batch_gpu(seeds: np.ndarray, blob: np.ndarray, msg_off: np.ndarray, msg_sz: np.ndarray, engine: Engine = None):
    """sign_batch on the GPU (fd_ed25519_gpu_sign_batch; engine None: the process-default
    engine), keys derived on the device: returns (pub[n,32], sig[n,64])."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
    n = len(seeds)
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64)
    msg_sz = np.ascontiguousarray(msg_sz, dtype=np.uint32)
    pub = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    err = lib().fd_ed25519_gpu_sign_batch(engine._h if engine is not None else None, n, _p(seeds), _p(blob), _p(msg_off),
                                          _p(msg_sz), _p(pub), _p(sig), 1)
    if err:
        raise EngineError(f"sign_batch_gpu: {strerror(err)}: {last_error()}")
    return pub, sig
