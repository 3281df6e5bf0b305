/* fd_txn_host.c -- Solana transaction wire parser (host side of the
   sigverify path).

   fd_txn_parse is the parser core (fd_txn_core.h: the cursor machine, the
   compact-u16 rules and the FD_TXN_REJ_* reference lines, shared with the
   device's fd_k_txn_parse) plus the reference's counters.  The output
   descriptor is byte-identical to the reference's fd_txn_t for every
   accepted payload, every rejected payload returns 0, and the counters
   match: each rejection records the reference's source line for that
   check, because the reference stores __LINE__ in its failure ring.
   Pinned by tests/test_txn.py against the reference parser compiled in
   place, over the fixtures, all truncations and all single-byte mutations
   (the reference's own test_mutate sweep,
   src/ballet/txn/test_txn_parse.c:107-190). */

#include <stddef.h>
#include "fd_txn_core.h"

#define FD_EXPORT __attribute__((visibility("default")))

FD_EXPORT unsigned long
fd_txn_parse( uint8_t const *           payload,
              unsigned long             payload_sz,
              void *                    out_buf,
              fd_txn_parse_counters_t * ctr ) {
  fd_txn_core_sum_t sum;
  unsigned long fp = fd_txn_core_parse( payload, payload_sz, out_buf, FD_TXN_CORE_CAP_TRUSTED, &sum );
  if( ctr ) {
    if( fp ) ctr->success_cnt++;
    else     ctr->failure_ring[ (ctr->failure_cnt++) % FD_TXN_PARSE_COUNTERS_RING_SZ ] = (unsigned long)sum.reject_line;
  }
  return fp;
}
