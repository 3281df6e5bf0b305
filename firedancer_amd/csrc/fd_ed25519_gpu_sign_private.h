/* fd_ed25519_gpu_sign_private.h -- launch prototypes of the signing
   kernels (fd_ed25519_gpu_sign_kernels.hip), shared with the host runtime. */
#ifndef FD_ED25519_GPU_SIGN_PRIVATE_H
#define FD_ED25519_GPU_SIGN_PRIVATE_H

#include <hip/hip_runtime.h>
#include "fd_ed25519_gpu_sign.h"

/* the inversion the library ships: 1 = Montgomery's trick over a wave's
   lanes, 0 = one inversion per lane (README, "Signing": the A/B) */
#ifndef FD_SGN_BATCH_INV
#define FD_SGN_BATCH_INV 0
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* fd_k_sign: n descriptors over blob[0, blob_sz); sig_out 64 n bytes,
   pub_out NULL or 32 n bytes (both 16-byte aligned), status n ints */
hipError_t fd_ed25519_gpu_launch_sign( uint64_t n, uint8_t const * blob, uint64_t blob_sz, fd_ed25519_gpu_sign_desc_t const * sdesc,
                                       uint8_t * sig_out, uint8_t * pub_out, int32_t * status, int batch_inv, hipStream_t stream );
/* fd_k_public: hash != 0: out = the public keys of n seeds; hash == 0
   (debug op 0): out = the encodings of [s]B for n raw scalars.  in and out
   32 n bytes, 16-byte aligned */
hipError_t fd_ed25519_gpu_launch_public( uint64_t n, uint8_t const * in, uint8_t * out, int hash, int batch_inv, hipStream_t stream );
/* fd_k_debug_muladd: out = (k a + r) mod L, 32 n bytes each, 8-byte aligned */
hipError_t fd_ed25519_gpu_launch_debug_muladd( uint64_t n, uint8_t const * k, uint8_t const * a, uint8_t const * r, uint8_t * out,
                                               hipStream_t stream );
#ifdef __cplusplus
}
#endif

#endif
