/* fd_ed25519_gpu_txn_private.h -- launch prototypes of the transaction
   kernels (fd_ed25519_gpu_txn_kernels.hip), shared with the host runtime. */
#ifndef FD_ED25519_GPU_TXN_PRIVATE_H
#define FD_ED25519_GPU_TXN_PRIVATE_H

#include <hip/hip_runtime.h>
#include "fd_ed25519_gpu_txn.h"

/* transactions per fd_k_txn_parse block: one partial sum of the scan */
#define FD_TXN_WG 256UL
/* n_txn bound of one launch: 127 signatures each still sum inside 32 bits */
#define FD_TXN_MAX (1UL<<24)

/* per transaction, between the kernels: x = signature count (0: takes no
   slot) | acct_addr_off << 16, y = the exclusive prefix of the counts
   inside its block */
typedef uint2 fd_txn_meta_t;

/* words of the scan's array for n_txn transactions: one partial per block,
   then the total, then the number of slots transactions took (n_sig) */
static inline unsigned long fd_txn_part_cnt( unsigned long n_txn ) { return (n_txn + FD_TXN_WG - 1UL) / FD_TXN_WG + 2UL; }

#ifdef __cplusplus
extern "C" {
#endif
/* fd_k_txn_parse, fd_k_txn_scan, fd_k_txn_expand on `stream`: results'
   parse fields, sig_base and the capacity verdict, the optional
   descriptors, slots [0, sig_cap) of desc and part[] as above.  ev: NULL,
   or 4 events recorded before and after each kernel. */
hipError_t fd_ed25519_gpu_launch_txn_front( uint64_t n_txn, uint8_t const * blob, uint64_t blob_sz, fd_ed25519_gpu_txn_t const * txn,
                                            uint64_t sig_cap, fd_ed25519_gpu_txn_result_t * res, uint8_t * txn_out,
                                            uint64_t txn_out_stride, fd_txn_meta_t * meta, uint32_t * part,
                                            fd_ed25519_gpu_desc_t * desc, hipStream_t stream, hipEvent_t const * ev );
/* fd_k_txn_reduce: status of every transaction that got slots */
hipError_t fd_ed25519_gpu_launch_txn_reduce( uint64_t n_txn, fd_ed25519_gpu_txn_result_t * res, int32_t const * codes,
                                             hipStream_t stream );
/* fd_k_txn_ring_front: the ring's one-launch front end.  bases[0..n_txn]
   is what fd_ed25519_gpu_txn_claims writes (n_sig = bases[n_txn]); res
   receives every field, status final for whatever did not parse; desc
   slots [0, n_sig). */
hipError_t fd_ed25519_gpu_launch_txn_ring_front( uint64_t n_txn, uint64_t n_sig, uint8_t const * blob, uint64_t blob_sz,
                                                 fd_ed25519_gpu_txn_t const * txn, uint32_t const * bases,
                                                 fd_ed25519_gpu_txn_result_t * res, fd_ed25519_gpu_desc_t * desc, hipStream_t stream );
/* fd_k_txn_ring_reduce: res folded with codes[0, n_sig) into out (mapped
   pinned memory, or anything else the device writes) */
hipError_t fd_ed25519_gpu_launch_txn_ring_reduce( uint64_t n_txn, uint64_t n_sig, fd_ed25519_gpu_txn_result_t const * res,
                                                  int32_t const * codes, fd_ed25519_gpu_txn_result_t * out, hipStream_t stream );
#ifdef __cplusplus
}
#endif

#endif
