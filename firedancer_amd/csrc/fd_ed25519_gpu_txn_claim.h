/* fd_ed25519_gpu_txn_claim.h -- signatures an entry claims (C and C++). */
#ifndef FD_ED25519_GPU_TXN_CLAIM_H
#define FD_ED25519_GPU_TXN_CLAIM_H

#include "fd_ed25519_gpu_txn.h"

/* signatures an entry claims: its first payload byte, if that can be read
   and is a count fd_txn_parse accepts; an upper bound on what it takes */
static inline unsigned long fd_txn_claim( uint8_t const * blob, unsigned long blob_sz, fd_ed25519_gpu_txn_t const * e ) {
  if( !e->sz || (unsigned long)e->off + (unsigned long)e->sz > blob_sz ) return 0UL;
  unsigned long c = blob[ e->off ];
  return ( c >= 1UL && c <= FD_TXN_SIG_MAX ) ? c : 0UL;
}

#endif
