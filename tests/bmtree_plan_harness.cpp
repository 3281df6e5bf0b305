/* bmtree_plan_harness.cpp -- the Merkle device call's plan arithmetic
   (fd_bmtree_gpu_private.h: fd_bmtree_plan_make, fd_bmtree_plan_layout,
   fd_bmtree_layer_bound, fd_bmtree_ceil_log2) on the host, exhaustively
   over small shapes.  tests/test_bmtree_plan_host.py builds it with
   UndefinedBehaviorSanitizer and compares the line it prints.

   Every multiset of tree sizes with N <= 40 leaves, with 0 and 3 more empty
   trees, with leaf_max in { 1, 2, 3, N-1, N, 2^30 }:
     lanes[l] is at least the exact node count of layer l+1,
     cap_a and cap_b are at least every layer they hold,
     L launches reach the root of every tree the count rules keep,
     bad | off | part | node_a | node_b are disjoint, 16-byte aligned, in
     this order, and end at the returned size.
   Then T = N = 0x7fffffff: no size wraps and every lane count fits 32 bits. */

#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "fd_bmtree_gpu_private.h"

static unsigned long n_multisets, n_plans, n_layers, n_tight[8];
alignas(16) static uint8_t small_work[ 1UL << 16 ];   /* the small plans are laid out in here; nothing is read or written */
static uint8_t * work = small_work;

#define CHECK(c) do { if( !(c) ) { \
  printf( "FAIL %s (line %d): T %lu N %lu leaf_max %lu sizes", #c, __LINE__, T, N, leaf_max ); \
  for( unsigned long s : sizes ) printf( " %lu", s ); \
  printf( "\n" ); exit( 1 ); } } while(0)

static void check_layout( fd_bmtree_plan_t const & p, unsigned long T, unsigned long N, unsigned long leaf_max, unsigned long sz,
                          std::vector<unsigned long> const & sizes ) {
  unsigned long rows = 0UL;
  while( ( 1UL << rows ) < N ) rows++;
  unsigned long NB = ( T + 255UL ) / 256UL;
  CHECK( fd_bmtree_ceil_log2( N ) == rows );
  CHECK( p.NB == NB && p.L <= rows );
  unsigned long at[6] = { (unsigned long)( (uint8_t *)p.bad - work ), (unsigned long)( (uint8_t *)p.off - work ),
                          (unsigned long)( (uint8_t *)p.part - work ), (unsigned long)( (uint8_t *)p.node_a - work ),
                          (unsigned long)( (uint8_t *)p.node_b - work ), sz };
  unsigned long need[5] = { 4UL*T, 4UL*rows*( T + 1UL ), 4UL*rows*NB, 32UL*(unsigned long)p.cap_a, 32UL*(unsigned long)p.cap_b };
  CHECK( at[0] == 0UL );
  for( int k=0; k<5; k++ ) {
    CHECK( !( at[k] & 15UL ) );
    CHECK( at[k] <= at[k+1] && at[k+1] - at[k] >= need[k] );
  }
  CHECK( !( sz & 15UL ) && sz - at[4] < 32UL*(unsigned long)p.cap_b + 16UL );
}

static void check_plan( std::vector<unsigned long> const & sizes, unsigned long empty, unsigned long leaf_max ) {
  unsigned long T = sizes.size() + empty, N = 0UL;
  for( unsigned long s : sizes ) N += s;
  if( !T ) return;
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, 32U, 0U, T, N, 0UL, leaf_max, work, lanes );
  fd_bmtree_plan_t q; memset( &q, 0, sizeof(q) ); q.T = (uint32_t)T; q.N = (uint32_t)N;
  unsigned long sz = fd_bmtree_plan_layout( &q, work );
  n_plans++;
  CHECK( p.T == T && p.N == N && p.leaf_max == leaf_max );
  CHECK( q.bad == p.bad && q.off == p.off && q.part == p.part && q.node_a == p.node_a && q.node_b == p.node_b );
  CHECK( q.cap_a == p.cap_a && q.cap_b == p.cap_b && q.NB == p.NB );
  check_layout( p, T, N, leaf_max, sz, sizes );
  CHECK( sz <= sizeof(small_work) );
  CHECK( p.cap_a >= N );                                 /* layer 0 */
  std::vector<unsigned long> c;
  for( unsigned long s : sizes ) if( s <= leaf_max ) c.push_back( s );
  for( uint32_t l=1U; ; l++ ) {                          /* layer l, written by launch l-1 */
    unsigned long exact = 0UL;
    for( unsigned long & x : c ) { x = x > 1UL ? ( x + 1UL ) >> 1 : 0UL; exact += x; }
    if( !exact ) break;
    CHECK( l <= p.L );                                   /* a layer past the launches: a root not reached */
    CHECK( (unsigned long)lanes[l-1U] == fd_bmtree_layer_bound( T, N, l ) );
    CHECK( (unsigned long)lanes[l-1U] >= exact );
    CHECK( exact <= ( ( l & 1U ) ? p.cap_b : p.cap_a ) );
    n_layers++;
    if( leaf_max == ( 1UL << 30 ) && !empty && lanes[l-1U] == exact && l < 8U ) n_tight[l]++;
  }
}

static void multisets( std::vector<unsigned long> & sizes, unsigned long left, unsigned long top ) {
  if( !left ) {
    unsigned long N = 0UL;
    for( unsigned long s : sizes ) N += s;
    n_multisets++;
    unsigned long lm[6] = { 1UL, 2UL, 3UL, N - 1UL, N, 1UL << 30 };
    for( unsigned long empty : { 0UL, 3UL } )
      for( int k=0; k<6; k++ ) {
        bool seen = !lm[k] || lm[k] > ( 1UL << 30 );   /* N - 1 of N = 0 or 1 is no leaf_max */
        for( int j=0; j<k; j++ ) seen = seen || lm[j] == lm[k];
        if( !seen ) check_plan( sizes, empty, lm[k] );
      }
    return;
  }
  for( unsigned long s = top < left ? top : left; s >= 1UL; s-- ) {
    sizes.push_back( s );
    multisets( sizes, left - s, s );
    sizes.pop_back();
  }
}

static int big( void ) {
  std::vector<unsigned long> sizes;
  unsigned long T = 0x7fffffffUL, N = 0x7fffffffUL, leaf_max = 1UL << 30;
  work = (uint8_t *)(uintptr_t)( 1UL << 20 );   /* an address, not an object: some 390 GB of offsets are only computed */
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, 20U, 0U, T, N, 0xffffffffUL, leaf_max, work, lanes );
  fd_bmtree_plan_t q; memset( &q, 0, sizeof(q) ); q.T = (uint32_t)T; q.N = (uint32_t)N;
  unsigned long sz = fd_bmtree_plan_layout( &q, work );
  CHECK( p.T == T && p.N == N && p.L == 30U && p.blob_sz == 0xffffffffU );
  CHECK( p.cap_a == N && (unsigned long)p.cap_b == 2UL*N/3UL + 1UL );
  check_layout( p, T, N, leaf_max, sz, sizes );
  unsigned __int128 low = (unsigned __int128)4*T + (unsigned __int128)4*31*( T + 1UL ) + (unsigned __int128)4*31*( ( T + 255UL ) / 256UL ) +
                          (unsigned __int128)32*N + (unsigned __int128)32*p.cap_b;
  CHECK( (unsigned __int128)sz >= low && (unsigned __int128)sz < low + 5*16 );
  for( uint32_t l=1U; l<=31U; l++ ) {
    unsigned __int128 act = (unsigned __int128)N / ( ( (unsigned __int128)1 << (l-1U) ) + 1 );
    unsigned __int128 want = ( (unsigned __int128)N >> l ) + ( act < T ? act : (unsigned __int128)T );
    CHECK( (unsigned __int128)fd_bmtree_layer_bound( T, N, l ) == want && want <= 0xffffffffUL );
    if( l <= p.L ) CHECK( (unsigned __int128)lanes[l-1U] == want );
  }
  return 1;
}

int main( void ) {
  std::vector<unsigned long> sizes;
  for( unsigned long N=0UL; N<=40UL; N++ ) multisets( sizes, N, N );
  int ok = big();
  printf( "multisets %lu plans %lu layers %lu tight", n_multisets, n_plans, n_layers );
  for( int l=1; l<=6; l++ ) printf( " %lu", n_tight[l] );
  printf( " big %s\n", ok ? "ok" : "FAIL" );
  return 0;
}
