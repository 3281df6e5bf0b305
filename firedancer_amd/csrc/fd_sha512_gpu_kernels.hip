/* fd_sha512_gpu_kernels.hip -- plain SHA-512 / SHA-384 of messages of any
   length (include/fd_sha512_gpu.h), streamed through the device in pieces.

   A translation unit of its own, outside the Makefile's KSRC: the verify
   kernels and their build id do not move with it.  It includes the verify
   path's SHA-512 header unchanged for fd_sha512_compress and the IVs.

   One lane per message, as fd_k_sha512_stream of the verify long path: the
   hash is serial within a message, so the parallelism is across the
   messages of a group.  What differs is the two ends: the stream starts
   from either IV with no R || A prefix, and its last piece leaves the
   finished big-endian digest in the lane's row, so the host moves bytes
   only. */

#include "fd_ed25519_gpu_sha512.h"
#include "fd_sha512_gpu_private.h"

extern "C" __global__ void __launch_bounds__(64)
fd_k_sha512_pieces( uint32_t n, uint64_t * __restrict__ st, uint8_t const * __restrict__ data,
                    fd_sha_lpiece_t const * __restrict__ pc ) {
  uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  fd_sha_lpiece_t p = pc[i];
  if( !p.nblk ) return;                      /* finished at an earlier launch: the row holds its digest */
  uint64_t * row = st + 8UL*(uint64_t)i;
  int iv = ( p.flags & FD_SHA_PIECE_384 ) ? 1 : 0;
  uint64_t s[8];
#pragma unroll
  for( int j=0; j<8; j++ ) s[j] = ( p.flags & FD_SHA_PIECE_FIRST ) ? fd_gpu_sha512_iv[iv][j] : row[j];
  ulonglong2 const * q = (ulonglong2 const *)(data + p.off);
  ulonglong2 cur[8];
#pragma unroll
  for( int c=0; c<8; c++ ) cur[c] = q[c];
  for( uint32_t b=0; b<p.nblk; b++ ) {
    uint64_t w[16];
#pragma unroll
    for( int c=0; c<8; c++ ) { w[2*c] = fd_bswap64( cur[c].x ); w[2*c+1] = fd_bswap64( cur[c].y ); }
    if( b + 1u < p.nblk ) {                  /* block b+1 is in flight while block b is compressed */
      q += 8;
#pragma unroll
      for( int c=0; c<8; c++ ) cur[c] = q[c];
    }
    fd_sha512_compress( s, w );
  }
  if( p.flags & FD_SHA_PIECE_LAST ) {
    int nw = iv ? 6 : 8;
#pragma unroll
    for( int j=0; j<8; j++ ) if( j < nw ) row[j] = fd_bswap64( s[j] );
  } else {
#pragma unroll
    for( int j=0; j<8; j++ ) row[j] = s[j];
  }
}

extern "C" hipError_t fd_sha512_gpu_launch_pieces( uint32_t n, uint64_t * st, uint8_t const * data, fd_sha_lpiece_t const * pieces,
                                                   hipStream_t stream ) {
  if( !n ) return hipSuccess;
  hipLaunchKernelGGL( fd_k_sha512_pieces, dim3((n + 63u) / 64u), dim3(64), 0, stream, n, st, data, pieces );
  return hipGetLastError();
}
