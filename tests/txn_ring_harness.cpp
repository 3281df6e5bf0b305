/* txn_ring_harness.cpp -- fd_ed25519_gpu_txn_claims (the claimed-slot rule
   of the ring's transaction batches) as a stand-alone host program, for
   AddressSanitizer and UndefinedBehaviorSanitizer
   (tests/test_txn_ring_host.py).  The routine's own source is compiled in.

   usage: txn_ring_harness CASES OUT
   CASES holds any number of cases, each
     u64 blob_sz | u64 n_txn | blob_sz bytes | n_txn entries (u32 off, u32 sz)
   and OUT receives, per case, u64 n_sig | n_txn + 1 u32 bases.  Each blob
   is copied to a heap block of exactly blob_sz bytes, the entries and the
   bases to blocks of exactly their sizes, so a read or write one byte
   outside any of them is caught.  Each case is also run with bases ==
   NULL (the total alone). */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_ed25519_gpu_txn_claims.c"

static int rd( FILE * f, void * p, size_t n ) { return n == 0 || fread( p, 1, n, f ) == n; }

int main( int argc, char ** argv ) {
  if( argc != 3 ) { fprintf( stderr, "usage: %s CASES OUT\n", argv[0] ); return 2; }
  FILE * in  = fopen( argv[1], "rb" );
  FILE * out = fopen( argv[2], "wb" );
  if( !in || !out ) { fprintf( stderr, "cannot open files\n" ); return 2; }
  unsigned long cases = 0UL, entries = 0UL;
  for(;;) {
    uint64_t hdr[2];
    size_t got = fread( hdr, 1, sizeof(hdr), in );
    if( got == 0 ) break;
    if( got != sizeof(hdr) ) { fprintf( stderr, "truncated header\n" ); return 2; }
    unsigned long blob_sz = (unsigned long)hdr[0], n_txn = (unsigned long)hdr[1];
    uint8_t *              blob  = (uint8_t *)malloc( blob_sz ? blob_sz : 1UL );
    fd_ed25519_gpu_txn_t * txn   = (fd_ed25519_gpu_txn_t *)malloc( n_txn ? n_txn * sizeof(fd_ed25519_gpu_txn_t) : 1UL );
    uint32_t *             bases = (uint32_t *)malloc( ( n_txn + 1UL ) * sizeof(uint32_t) );
    if( !blob || !txn || !bases ) { fprintf( stderr, "out of memory\n" ); return 2; }
    if( !rd( in, blob, blob_sz ) || !rd( in, txn, n_txn * sizeof(fd_ed25519_gpu_txn_t) ) ) { fprintf( stderr, "truncated case\n" ); return 2; }
    /* blob_sz == 0: the one byte that malloc gave is not the blob's */
    uint64_t n_sig = fd_ed25519_gpu_txn_claims( blob_sz ? blob : NULL, blob_sz, txn, n_txn, bases );
    uint64_t again = fd_ed25519_gpu_txn_claims( blob_sz ? blob : NULL, blob_sz, txn, n_txn, NULL );
    if( n_sig != again || bases[ n_txn ] != (uint32_t)n_sig ) { fprintf( stderr, "case %lu: totals differ\n", cases ); return 1; }
    fwrite( &n_sig, 1, sizeof(n_sig), out );
    fwrite( bases, 1, ( n_txn + 1UL ) * sizeof(uint32_t), out );
    free( blob ); free( txn ); free( bases );
    cases++; entries += n_txn;
  }
  fclose( in );
  if( fclose( out ) ) { fprintf( stderr, "write failed\n" ); return 2; }
  printf( "%lu cases, %lu entries ok\n", cases, entries );
  return 0;
}
