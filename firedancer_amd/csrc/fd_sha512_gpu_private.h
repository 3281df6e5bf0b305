/* fd_sha512_gpu_private.h -- launch prototype of the long plain-hash kernel
   (fd_sha512_gpu_kernels.hip), shared with the host runtime. */
#ifndef FD_SHA512_GPU_PRIVATE_H
#define FD_SHA512_GPU_PRIVATE_H

#include <hip/hip_runtime.h>
#include "fd_sha512_gpu.h"
#include "fd_sha512_gpu_pack.h"

/* the long runner's buffering: 1 = the pinned blob as two halves, one
   packed while the device hashes the other; 0 = one buffer, a wait per
   launch.  The library ships 0: in seven alternating pairs at 4,096
   messages of 256 KB the two halves were no faster (0.288-0.293 s against
   0.288-0.301 s per fini), and the rule was that ping-pong ships only if
   every one of its runs beats every single-buffer run (DESIGN section 7e:
   the A/B) */
#ifndef FD_SHA_LONG_PINGPONG
#define FD_SHA_LONG_PINGPONG 0
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* fd_k_sha512_pieces: lane i < n compresses pieces[i].nblk blocks at
   data + pieces[i].off (16-byte aligned) into row st[8 i .. 8 i + 8): from
   the IV on FIRST, else from the row; nblk 0 leaves the row alone; on LAST
   the row receives the big-endian digest (8 words, 6 for SHA-384) */
hipError_t fd_sha512_gpu_launch_pieces( uint32_t n, uint64_t * st, uint8_t const * data, fd_sha_lpiece_t const * pieces,
                                        hipStream_t stream );

/* The long runner (fd_ed25519_gpu_host.cpp): the digests of cnt messages of
   any size, each written to its own hash pointer (64 bytes, is384: 48),
   through one staged slot of the ring.  Returns 0, FD_ED25519_ERR_GPU
   (device error or timeout) or FD_ED25519_ERR_ARG (a blob below 144 bytes,
   which cannot hold one block and its piece entry). */
typedef struct { void const * data; unsigned long sz; void * hash; } fd_sha_long_req_t;
int fd_sha512_gpu_long( fd_ed25519_gpu_t * gpu, unsigned long cnt, fd_sha_long_req_t const * rq, int is384 );
#ifdef __cplusplus
}
#endif

#endif
