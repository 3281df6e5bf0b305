#ifndef HEADER_fd_ed25519_gpu_sign_h
#define HEADER_fd_ed25519_gpu_sign_h

/* fd_ed25519_gpu_sign.h -- batch Ed25519 signing and key derivation on the
   GPU engine (RFC 8032 5.1.5 / 5.1.6; the reference's contract
   src/ballet/ed25519/fd_ed25519.h:40-73).

   One lane per signature: az = SHA-512(seed), r = SHA-512(az[32..64) || M)
   mod L, R = [r]B by a fixed-base comb, k = SHA-512(R || A || M) mod L,
   S = (k a + r) mod L.  Outputs are deterministic and byte-identical to
   fd_ed25519_sign / fd_ed25519_public_from_private.

   Which signer to call: the per-call fd_ed25519_sign and
   fd_ed25519_public_from_private (fd_ed25519_gpu.h) stay on the host --
   one call is tens of microseconds there against a 0.35 ms device round
   trip.  The batch entry points below are for thousands of signatures at
   once (corpus generation, load generators, a validator's shred / vote /
   gossip bursts).

   Seeds on the device: the packed calls stage seeds in the engine's pinned
   and device slot buffers and clear both after the batch (also when it
   fails or times out: an orphaned slot is cleared by the same stream
   before it can be reused).  The kernels keep az, a and r in registers
   only.  The device-resident call works on the caller's memory and clears
   nothing there. */

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One signature to make: the 32-byte seed (private key) at
   blob[seed_off..+32), the message at blob[msg_off..+msg_sz), and the
   public key either at blob[pub_off..+32) or, with pub_off =
   FD_ED25519_GPU_SIGN_DERIVE, derived from the seed on the device.  A key
   given at pub_off is used as is in SHA-512(R || A || M); it is never
   checked against the seed (the reference's contract: a wrong key yields
   the bytes the host signer yields for that wrong key).  16 bytes, as
   fd_ed25519_gpu_desc_t. */
typedef struct { uint32_t seed_off, pub_off, msg_off, msg_sz; } fd_ed25519_gpu_sign_desc_t;
#define FD_ED25519_GPU_SIGN_DERIVE (0xffffffffU)

/* pub_out[32 i ..) = the public key of seeds[32 i ..), i < n <= max_sigs.
   Synchronous, host buffers.  Returns 0, FD_ED25519_ERR_ARG (NULL array,
   n > max_sigs; nothing is sent to the device) or FD_ED25519_ERR_GPU
   (device failure or timeout; nothing written). */
int
fd_ed25519_gpu_public_packed( fd_ed25519_gpu_t * gpu,
                              unsigned long      n,
                              void const *       seeds,
                              void *             pub_out );

/* Sign n packed descriptors.  sig_out[64 i ..) = R || S; pub_out_opt (NULL
   or 32 n bytes) receives the key each signature was made with (derived or
   given); out[i] = FD_ED25519_SUCCESS, or FD_ED25519_ERR_ARG for a
   descriptor whose seed, key or message does not lie inside
   blob[0, blob_sz): that entry is never dereferenced and gets 64 zero
   bytes (32 in pub_out_opt).  Synchronous, host buffers.  Returns 0,
   FD_ED25519_ERR_ARG (n > max_sigs, blob_sz > max_blob, a NULL array;
   nothing is sent to the device) or FD_ED25519_ERR_GPU (device failure or
   timeout; nothing written). */
int
fd_ed25519_gpu_sign_packed( fd_ed25519_gpu_t *                 gpu,
                            unsigned long                      n,
                            void const *                       blob,
                            unsigned long                      blob_sz,
                            fd_ed25519_gpu_sign_desc_t const * sdesc,
                            void *                             sig_out,
                            void *                             pub_out_opt,
                            int *                              out );

/* Device-resident: d_blob (blob_sz bytes followed by >= 16 readable pad
   bytes, 4-byte aligned), d_sdesc, d_sig_out (64 n bytes, 16-byte
   aligned), d_pub_out_opt (NULL or 32 n bytes, 16-byte aligned) and d_out
   (n ints) are device pointers.  The stream contract of
   fd_ed25519_gpu_verify_dev: the work is ordered after everything queued
   on `stream` (NULL: the engine's own) and its results are visible to work
   queued on `stream` afterwards; no host synchronisation.  blob_sz is not
   bounded by max_blob and n not by max_sigs (no engine scratch is used).
   The memory is the caller's: seeds in d_blob are NOT cleared. */
int
fd_ed25519_gpu_sign_dev( fd_ed25519_gpu_t *                 gpu,
                         unsigned long                      n,
                         void const *                       d_blob,
                         unsigned long                      blob_sz,
                         fd_ed25519_gpu_sign_desc_t const * d_sdesc,
                         void *                             d_sig_out,
                         void *                             d_pub_out_opt,
                         int *                              d_out,
                         void *                             stream );

/* fd_ed25519_sign_batch (seed[32 i ..), message blob[msg_off[i]..
   +msg_sz[i]), pub[32 i ..), sig[64 i ..)) on an engine (NULL: the process
   default), in engine-sized chunks.  derive != 0: pub is an output,
   derived on the device; derive == 0: pub is an input, used as given.  A
   message that does not fit the engine's staging blob is signed by the
   host routine for that element (no device long-message signing).  Returns
   0, or FD_ED25519_ERR_ARG / FD_ED25519_ERR_GPU with sig (and a derived
   pub) incomplete. */
int
fd_ed25519_gpu_sign_batch( fd_ed25519_gpu_t *    gpu,
                           unsigned long         n,
                           unsigned char const * seed,
                           unsigned char const * blob,
                           uint64_t const *      msg_off,
                           uint32_t const *      msg_sz,
                           unsigned char *       pub,
                           unsigned char *       sig,
                           int                   derive );

/* the same on the process-default engine */
int
fd_ed25519_sign_batch_gpu( unsigned long         n,
                           unsigned char const * seed,
                           unsigned char const * blob,
                           uint64_t const *      msg_off,
                           uint32_t const *      msg_sz,
                           unsigned char *       pub,
                           unsigned char *       sig,
                           int                   derive );

/* Diagnostics, in the style of fd_ed25519_gpu_debug_fe: inputs a test can
   choose freely where the hash-derived r never lets it.
     op 0: out[32 i ..) = the encoding of [s]B, s = in0[32 i ..) any 256-bit
           little-endian scalar (in1, in2 unused)
     op 1: out[32 i ..) = (k a + r) mod L, k = in0, a = in1, r = in2
           (32 bytes each; k, r < L, a < 2^255)
   Synchronous, host buffers, n <= 2^20. */
int
fd_ed25519_gpu_debug_sign_op( fd_ed25519_gpu_t * gpu,
                              int                op,
                              unsigned long      n,
                              void const *       in0,
                              void const *       in1,
                              void const *       in2,
                              void *             out );

/* Experiments (tools/sign_bench.py): the point encodings' inversion, 0 =
   one fd_fe_invert per lane, 1 = Montgomery's trick over the lanes of a
   wave.  The library's default is the compile-time FD_SGN_BATCH_INV.
   Process-wide; returns the previous value. */
int fd_ed25519_gpu_sign_set_batch_inv( int on );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_gpu_sign_h */
