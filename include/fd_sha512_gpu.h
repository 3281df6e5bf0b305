#ifndef HEADER_fd_sha512_gpu_h
#define HEADER_fd_sha512_gpu_h

/* fd_sha512_gpu.h -- GPU backend for the ballet SHA-512 batch API
   (SURVEY.md section 8f row 3).

   The reference's batch API (src/ballet/sha512/fd_sha512.h:223-294) is
   header-inline: add() queues (data, sz, hash) and hashes 4 at a time
   with AVX2; fini() flushes.  The GPU backend keeps the same contract --
   after fini every queued hash[i] holds SHA-512(data[i][0..sz)), data
   must stay valid until fini, abort drops the queue -- but queues
   without limit and hashes everything in one device pass per engine
   batch (one lane per message, the sigverify path's SHA-512 core).
   INTEGRATION.md shows the fd_sha512.h branch that selects it.

   There is no restriction on sz, as in the reference
   (src/ballet/sha256/fd_sha256.h:191-192, which fd_sha512.h:221 points
   to): a message larger than the engine's staging blob, or than the
   2^32 - 1 bytes a descriptor addresses, is streamed through the blob in
   pieces, one lane per message and several messages side by side
   (fd_k_sha512_pieces), the chaining state kept on the device between
   launches.  The hash is serial within a message, so one very long message
   runs at a single lane's rate.

   fd_sha384 variants (fd_sha512.h:150-222) use the SHA-384 IV and write
   48 bytes.  There is no CPU fallback: on engine failure (a device error
   or a wait past the engine's timeout) fini returns NULL.  The one input
   it cannot hash: a message larger than the blob of an engine whose blob
   is below 144 bytes, which cannot hold a single 128-byte block and its
   16-byte piece entry. */

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device digests of packed messages: n digests of 64 (is384: 48) bytes,
   back to back, for blob[desc[i].msg_off .. +desc[i].msg_sz).  Returns 0,
   FD_ED25519_ERR_ARG (bounds / capacity) or FD_ED25519_ERR_GPU. */
int
fd_ed25519_gpu_sha512_packed( fd_ed25519_gpu_t *            gpu,
                              unsigned long                 n,
                              void const *                  blob,
                              unsigned long                 blob_sz,
                              fd_ed25519_gpu_desc_t const * desc,
                              void *                        hash_out,
                              int                           is384 );

/* Digests of n messages data[i][0..sz[i]) of any size, written back to
   back (64 bytes each, is384: 48) to hash_out; any n.  data[i] may be NULL
   where sz[i] is 0.  Messages that fit the engine's blob go through staged
   fd_ed25519_gpu_sha512_packed chunks, the others through the long path
   above.  gpu may be NULL: the process-default engine.  Returns 0,
   FD_ED25519_ERR_ARG (a NULL array or message; the degenerate blob above)
   or FD_ED25519_ERR_GPU (no device, device error, timeout). */
int
fd_ed25519_gpu_sha512_ptrs( fd_ed25519_gpu_t *    gpu,
                            unsigned long         n,
                            void const * const *  data,
                            unsigned long const * sz,
                            void *                hash_out,
                            int                   is384 );

/* Diagnostic: how the long path moves a group of m messages through a
   pinned blob of max_blob bytes on an engine of max_sigs.  *G: messages
   hashed side by side in a group, at most min( max_sigs, 4096 ); *C: the
   128-byte blocks per message per launch, >= 1.  A buffer is m C 128 data
   bytes followed by its m 16-byte piece entries.  The library as shipped
   uses the whole blob as one buffer; a build with FD_SHA_LONG_PINGPONG=1
   splits it into two such halves, one packed while the device hashes the
   other (a blob below 288 bytes, too small for two halves of one message,
   stays one buffer), and this function reports the geometry of the build
   it is in.  Pure arithmetic, no device.  Returns 0, or FD_ED25519_ERR_ARG
   if m is not in [1, *G] -- *G is 0 exactly for the blob below 144 bytes
   that cannot hold one block and its entry (or max_sigs 0). */
int
fd_sha512_gpu_long_geometry( unsigned long   max_blob,
                             unsigned long   max_sigs,
                             unsigned long   m,
                             unsigned long * G,
                             unsigned long * C );

typedef struct fd_sha512_gpu_batch fd_sha512_gpu_batch_t;

/* gpu may be NULL: the process-default engine (as fd_ed25519_verify). */
fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_new   ( fd_ed25519_gpu_t * gpu, int is384 );
void                    fd_sha512_gpu_batch_delete( fd_sha512_gpu_batch_t * batch );

fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_init ( fd_sha512_gpu_batch_t * batch );
fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_add  ( fd_sha512_gpu_batch_t * batch,
                                                   void const *            data,
                                                   unsigned long           sz,
                                                   void *                  hash );
void *                  fd_sha512_gpu_batch_fini ( fd_sha512_gpu_batch_t * batch );
void *                  fd_sha512_gpu_batch_abort( fd_sha512_gpu_batch_t * batch );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_sha512_gpu_h */
