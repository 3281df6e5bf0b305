/* poh_core_harness.cpp -- the Proof-of-History host routines
   (firedancer_amd/csrc/fd_poh_host.c over fd_poh_core.h) as a stand-alone
   program, built by tests/test_poh_core_sanitize.py under AddressSanitizer
   and UndefinedBehaviorSanitizer.

   Each argument is a case file written by the test from hashlib's results:
     u64 count, u64 n_max, count entries (112 bytes), count i32 codes,
     count 32-byte states
   The entries are copied to a heap block of exactly their size and the
   outputs go to blocks of exactly theirs, so a read or write one byte past
   either is caught.  Every file goes through fd_poh_verify_batch (1 and 4
   threads, with and without states) and, entry by entry, through
   fd_poh_append and fd_poh_mixin; fd_poh_gpu_chain is checked on the
   entries' own hashes. */

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "fd_poh_gpu.h"

#define CHECK(c) do { if( !(c) ) { fprintf( stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c ); return 1; } } while(0)

static int run_file( char const * path, unsigned long * total ) {
  FILE * f = fopen( path, "rb" );
  CHECK( f );
  uint64_t hdr[2];
  CHECK( fread( hdr, 8, 2, f ) == 2 );
  unsigned long cnt = hdr[0], n_max = hdr[1];
  CHECK( cnt && cnt < (1UL<<20) );
  fd_poh_gpu_entry_t * ent = (fd_poh_gpu_entry_t *)malloc( cnt * sizeof(fd_poh_gpu_entry_t) );
  int *     codes  = (int *)malloc( cnt * sizeof(int) );
  uint8_t * states = (uint8_t *)malloc( cnt * 32UL );
  int *     out    = (int *)malloc( cnt * sizeof(int) );
  uint8_t * st     = (uint8_t *)malloc( cnt * 32UL );
  CHECK( ent && codes && states && out && st );
  CHECK( fread( ent, sizeof(fd_poh_gpu_entry_t), cnt, f ) == cnt );
  CHECK( fread( codes, sizeof(int), cnt, f ) == cnt );
  CHECK( fread( states, 32, cnt, f ) == cnt );
  fclose( f );

  for( int th=1; th<=4; th+=3 ) {
    memset( out, 0x55, cnt * sizeof(int) ); memset( st, 0x55, cnt * 32UL );
    CHECK( !fd_poh_verify_batch( cnt, ent, n_max, out, st, th ) );
    CHECK( !memcmp( out, codes, cnt * sizeof(int) ) );
    CHECK( !memcmp( st, states, cnt * 32UL ) );
    memset( out, 0x55, cnt * sizeof(int) );
    CHECK( !fd_poh_verify_batch( cnt, ent, n_max, out, NULL, th ) );
    CHECK( !memcmp( out, codes, cnt * sizeof(int) ) );
  }

  for( unsigned long i=0; i<cnt; i++ ) {
    if( codes[i] == FD_ED25519_ERR_ARG ) continue;
    fd_poh_state_t s;
    memcpy( s.state, ent[i].start, 32 );
    CHECK( fd_poh_append( &s, ent[i].n ) == &s );
    if( ent[i].flags & FD_POH_GPU_MIXIN ) {
      uint8_t * mx = (uint8_t *)malloc( 32 );      /* a mixin with nothing after it */
      CHECK( mx );
      memcpy( mx, ent[i].mixin, 32 );
      CHECK( fd_poh_mixin( &s, mx ) == &s );
      free( mx );
    }
    CHECK( !memcmp( s.state, states + 32UL*i, 32 ) );
  }

  {
    std::vector<fd_poh_gpu_entry_t> run( cnt );
    uint8_t seed[32];
    memset( seed, 0xa5, 32 );
    fd_poh_gpu_chain( cnt, seed, states, run.data() );
    for( unsigned long i=0; i<cnt; i++ ) {
      CHECK( !memcmp( run[i].start,  i ? states + 32UL*(i-1UL) : seed, 32 ) );
      CHECK( !memcmp( run[i].expect, states + 32UL*i, 32 ) );
    }
  }

  free( ent ); free( codes ); free( states ); free( out ); free( st );
  *total += cnt;
  return 0;
}

int main( int argc, char ** argv ) {
  unsigned long total = 0UL;
  for( int a=1; a<argc; a++ ) if( run_file( argv[a], &total ) ) return 1;
  printf( "%lu entries ok\n", total );
  return 0;
}
