/* fd_ed25519_gpu_txn_claims.c -- the claimed-slot rule of the ring's
   transaction batches (include/fd_ed25519_gpu_txn.h) as plain host C: no
   engine, no device, no libc.  A unit of its own so that a tile, and the
   sanitizer harness (tests/txn_ring_harness.cpp), can use it without the
   HIP runtime. */

#include "fd_ed25519_gpu_txn_claim.h"

#define FD_EXPORT __attribute__((visibility("default")))

FD_EXPORT unsigned long
fd_ed25519_gpu_txn_claims( void const *                 blob,
                           unsigned long                blob_sz,
                           fd_ed25519_gpu_txn_t const * txn,
                           unsigned long                n_txn,
                           uint32_t *                   bases ) {
  unsigned long sum = 0UL;
  for( unsigned long t=0UL; t<n_txn; t++ ) {
    if( bases ) bases[ t ] = (uint32_t)sum;
    sum += fd_txn_claim( (uint8_t const *)blob, blob_sz, txn + t );
  }
  if( bases ) bases[ n_txn ] = (uint32_t)sum;
  return sum;
}
