// fe_mul_one_host.cpp -- stand-alone host program: fd_fe_mul_one( f ) against
// fd_fe_mul( f, one ) (firedancer_amd/csrc/fd_ed25519_gpu_fe.h, __host__
// __device__), limb for limb, over seeded inputs.  fd_fe_mul itself is held
// to the reference's AVX field path by tests/test_fe_host.py.  Prints one
// line per input class and exits nonzero at the first class with a
// mismatch (tests/test_fe_mul_one_host.py).  Test infrastructure only.
#include "fd_ed25519_gpu_fe.h"
#include <stdio.h>

typedef fd_gpu_fe_t fe;

static uint64_t rng_state;
static uint64_t rnd( void ) {   /* splitmix64 */
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
/* uniform in [-2^(bits-1), 2^(bits-1)) */
static int32_t rnd_bits( int bits ) { return (int32_t)(rnd() & ((1ULL<<bits)-1ULL)) - (int32_t)(1LL<<(bits-1)); }

/* a carried limb vector: what a product leaves (|even| <= 2^25, |odd| <= 2^24,
   limbs 1 and 5 a little past it) */
static void carried( fe & f ) {
  for( int k=0; k<10; k++ ) f.v[k] = rnd_bits( (k&1) ? 25 : 26 ) + (int32_t)((k==1 || k==5) ? rnd_bits( 12 ) : 0);
}

static int check( fe const & f, unsigned long & bad ) {
  fe one, a, b;
  fd_fe_set( one, 1 );
  fd_fe_mul( a, f, one );
  fd_fe_mul_one( b, f );
  int ok = 1;
  for( int k=0; k<10; k++ ) ok &= (a.v[k] == b.v[k]);
  if( !ok && !bad++ ) {
    printf( "first mismatch: f =" );   for( int k=0; k<10; k++ ) printf( " %d", f.v[k] );
    printf( "\n  fd_fe_mul     =" );   for( int k=0; k<10; k++ ) printf( " %d", a.v[k] );
    printf( "\n  fd_fe_mul_one =" );   for( int k=0; k<10; k++ ) printf( " %d", b.v[k] );
    printf( "\n" );
  }
  return ok;
}

int main( void ) {
  unsigned long const N = 40000UL;
  unsigned long total = 0UL, bad_total = 0UL;
  rng_state = 20240607ULL;

  /* 1. carried limbs */
  { unsigned long bad = 0UL;
    for( unsigned long i=0; i<N; i++ ) { fe f; carried( f ); check( f, bad ); }
    printf( "carried   %lu inputs, %lu mismatches\n", N, bad ); total += N; bad_total += bad; }

  /* 2. the unreduced sums the Ai precompute feeds in: the lanes of
        v_sub_mix [c-b, c+b, 2a-d, 2a+d] and v_subadd_12 [b-c, b+c] over
        carried a, b, c, d, and the negated coordinates of -A */
  { unsigned long bad = 0UL, cnt = 0UL;
    for( unsigned long i=0; i<N/8UL; i++ ) {
      fe a, b, c, d, f[8];
      carried( a ); carried( b ); carried( c ); carried( d );
      for( int k=0; k<10; k++ ) {
        uint32_t ua = (uint32_t)a.v[k], ub = (uint32_t)b.v[k], uc = (uint32_t)c.v[k], ud = (uint32_t)d.v[k];
        f[0].v[k] = (int32_t)(uc-ub);    f[1].v[k] = (int32_t)(uc+ub);
        f[2].v[k] = (int32_t)(2u*ua-ud); f[3].v[k] = (int32_t)(2u*ua+ud);
        f[4].v[k] = (int32_t)(ub-uc);    f[5].v[k] = (int32_t)(ub+uc);
        f[6].v[k] = (int32_t)(0u-ua);    f[7].v[k] = (int32_t)(0u-(2u*ua+ud));
      }
      for( int j=0; j<8; j++ ) { check( f[j], bad ); cnt++; }
    }
    printf( "unreduced %lu inputs, %lu mismatches\n", cnt, bad ); total += cnt; bad_total += bad; }

  /* 3. limbs at 0, +-1, +-2^25, +-2^26 and the int32 extremes (and one off
        each: the carry rounding boundaries), every limb drawn on its own;
        first every edge value in all ten limbs at once */
  { static int32_t const E[] = { 0, 1, -1, 1<<25, -(1<<25), 1<<26, -(1<<26), INT32_MAX, INT32_MIN,
                                 (1<<25)-1, -(1<<25)-1, (1<<25)+1, (1<<26)-1, (1<<26)+1, -(1<<26)-1, 1<<24, -(1<<24), (1<<24)-1,
                                 INT32_MAX-1, INT32_MIN+1 };
    unsigned long const ne = sizeof(E)/sizeof(E[0]);
    unsigned long bad = 0UL, cnt = 0UL;
    for( unsigned long e=0; e<ne; e++ ) { fe f; for( int k=0; k<10; k++ ) f.v[k] = E[e]; check( f, bad ); cnt++; }
    for( unsigned long e=0; e<ne; e++ ) for( int k=0; k<10; k++ ) {   /* one edge limb among zeros */
      fe f; fd_fe_set( f, 0 ); f.v[k] = E[e]; check( f, bad ); cnt++;
    }
    for( unsigned long i=0; i<N; i++ ) { fe f; for( int k=0; k<10; k++ ) f.v[k] = E[ rnd() % ne ]; check( f, bad ); cnt++; }
    printf( "edges     %lu inputs, %lu mismatches\n", cnt, bad ); total += cnt; bad_total += bad; }

  /* 4. any int32 limbs (the 32-bit wrap of the operand pre-scales) */
  { unsigned long bad = 0UL;
    for( unsigned long i=0; i<N; i++ ) { fe f; for( int k=0; k<10; k++ ) f.v[k] = (int32_t)(uint32_t)rnd(); check( f, bad ); }
    printf( "int32     %lu inputs, %lu mismatches\n", N, bad ); total += N; bad_total += bad; }

  printf( "total     %lu inputs, %lu mismatches\n", total, bad_total );
  return bad_total ? 1 : 0;
}
