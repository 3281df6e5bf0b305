#ifndef HEADER_fd_ed25519_gpu_diag_h
#define HEADER_fd_ed25519_gpu_diag_h

/* fd_ed25519_gpu_diag.h -- engine diagnostics for harnesses and
   operators (no reference counterpart; the reference's accelerator
   interface exposes no queue state either, src/wiredancer/c/wd_f1.h).
   Kept apart from fd_ed25519_gpu.h, which the device code includes: a
   declaration here does not change the kernels' build id
   (fd_ed25519_gpu_kernels_id). */

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ring slots' states (e.g. for a harness that outlived its time limit):
   out[s] for s < min(depth, max) is a bit set -- 1 holds a ticket, 2
   staged (lent to a caller), 4 retiring (codes taken early), 8 orphaned,
   16 early codes, 32 its completion event has fired.  Taken under the
   ring lock.  Returns the number of slots written. */
int fd_ed25519_gpu_slot_states( fd_ed25519_gpu_t * gpu, int * out, int max );

/* Verify n signatures with each one's 64-byte digest supplied by the
   caller in place of SHA-512(R || A || M): dig[64 i .. 64 i + 64) is the
   byte string the reference hands to fd_ed25519_sc_reduce
   (fd_ed25519_user.c:411-414), i.e. the digest in SHA-512's output byte
   order, read as a 512-bit little-endian integer and reduced mod L to give
   k.  (The host turns it into the chaining-state words fd_k_prep_dig
   loads: word j is the big-endian read of bytes 8j .. 8j+7.)  The message
   bytes are not read; msg_sz may be 0.

   Everything after the digest is the product path: the S range check,
   point decompression, the small-order flags, the double-scalar
   multiplication on the schedule (uniform, pooled, quad, oct) that the
   engine's mode and dsm_pool_min / dsm_quad_max / dsm_oct_max knobs give
   a batch of n, the compare and the code precedence, with ERR_ARG for
   descriptors outside the blob.  With k chosen freely a harness can build
   a valid signature at any (S, k): pick a, set A = [a]B and
   R = [S - k a mod L]B.

   blob / desc as fd_ed25519_gpu_verify_packed (host memory).  codes_out
   receives n codes.  k_out (n x 32 bytes) receives k little endian and
   status_out[i] is 1 for the signatures still pending after the S check;
   the others (and malformed descriptors) get 32 zero bytes and a status
   != 1, as fd_ed25519_gpu_debug_k reports them.  k_out and status_out may
   be NULL.  Synchronous.  Returns 0, FD_ED25519_ERR_ARG (NULL arguments,
   n > max_sigs, blob_sz > max_blob) or FD_ED25519_ERR_GPU; n == 0 returns
   0 and writes nothing. */
int fd_ed25519_gpu_debug_verify_dig( fd_ed25519_gpu_t * gpu, unsigned long n, void const * blob, unsigned long blob_sz,
                                     fd_ed25519_gpu_desc_t const * desc, unsigned char const * dig,
                                     int * codes_out, unsigned char * k_out, int * status_out );

/* One verify launch of n signatures with the stages it leaves in the
   engine's HBM working set read back, so a harness can hold each stage of
   the device code to the reference limb for limb instead of through the
   final code alone.  Host code only: the kernels are the product's.

   blob / desc as fd_ed25519_gpu_verify_packed (host memory).  dig NULL:
   the product's front end (real SHA-512; on the latency schedules the
   fused front-end kernel with its S digits recoded ahead for n <= 32).
   dig given (n x 64 bytes, as fd_ed25519_gpu_debug_verify_dig): the
   chosen-digest front end.  The back end, the mode and the schedule the
   dsm_pool_min / dsm_quad_max / dsm_oct_max knobs give a batch of n are
   the product's in both cases.

   Every output may be NULL; each is read after the back end ran, except
   status, which is prep's (taken before the DSM):
     codes_out    [n]           the codes
     status_out   [n]           prep's status (1: pending after the S check)
     pstat_out    [2n]          point status, A rows then R rows
                                (0 ok, 1 not on the curve, 2 small order)
     pts_out      [2n][40]      X, Y, Z, T limbs per point, A rows then R
                                rows (the device keeps them [40][2n]); a
                                row is written only where the front end
                                decoded the point
     op_start_out [n]           first op of the stream (512: no stream)
     ops_out      [n][512]      the op stream, signature-major whichever
                                layout the device used; on the latency
                                schedules only pending rows are written
     tab_out      [n][8][4][12] the Ai table, raw dwords with each lane's
                                two pad dwords (the pooled schedule keeps
                                it [entry][n]); written only if info_out[2]
     fin_out      [n][40]       the pooled DSM's final p1p1 rows; written
                                only if info_out[3]
     info_out     [4]           [0] schedule (FD_ED25519_GPU_SCHED_*),
                                [1] 1 if the device's op array was
                                signature-major, 0 step-major, [2] 1 if the
                                schedule writes an Ai table to HBM, [3] 1
                                if it writes final rows (pooled only)
   Rows of signatures that left the pipeline earlier hold whatever an
   earlier launch left there.  Synchronous.  Returns 0,
   FD_ED25519_ERR_ARG (NULL engine, NULL desc with n > 0, n > max_sigs,
   blob_sz > max_blob) or FD_ED25519_ERR_GPU; n == 0 returns 0 and writes
   nothing. */
#define FD_ED25519_GPU_SCHED_UNIFORM 0
#define FD_ED25519_GPU_SCHED_POOLED  1
#define FD_ED25519_GPU_SCHED_QUAD    2
#define FD_ED25519_GPU_SCHED_OCT     3
int fd_ed25519_gpu_debug_stages( fd_ed25519_gpu_t * gpu, unsigned long n, void const * blob, unsigned long blob_sz,
                                 fd_ed25519_gpu_desc_t const * desc, unsigned char const * dig,
                                 int * codes_out, int * status_out, int * pstat_out, int * pts_out,
                                 int * op_start_out, unsigned char * ops_out, int * tab_out, int * fin_out,
                                 int * info_out );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_gpu_diag_h */
