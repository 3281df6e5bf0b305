// sign_host_harness.cpp -- runs the signing core of
// firedancer_amd/csrc/fd_ed25519_gpu_sign_core.h (whose functions are
// __host__ __device__) on the host CPU, so tests/test_sign_host.py can hold
// it against a big-integer model and the oracle's signer before it reaches
// the GPU.  The wave's lane exchange of the batched inversion is an array
// here.  With -DSIGN_HARNESS_MAIN it is a stand-alone program that runs the
// edge cases (tests/test_sign_sanitize.py builds that with sanitizers).
// Test infrastructure only.
#include <stdio.h>
#include <string.h>
#include "fd_ed25519_gpu_sign_core.h"
#include "fd_ed25519_sign_tables.h"

static_assert( FD_SGN_TAB_ENTRIES == FD_SGN_COMB_ENTS && FD_SGN_TAB_ENTRY_DW == FD_SGN_COMB_DW, "comb geometry" );

typedef int const * tabp;

static void ld_words( uint32_t (&w)[8], uint8_t const * p ) {
  for( int j=0; j<8; j++ ) w[j] = (uint32_t)p[4*j] | ((uint32_t)p[4*j+1]<<8) | ((uint32_t)p[4*j+2]<<16) | ((uint32_t)p[4*j+3]<<24);
}
static void st_words( uint8_t * p, uint32_t const (&w)[8] ) {
  for( int j=0; j<8; j++ ) for( int b=0; b<4; b++ ) p[4*j+b] = (uint8_t)(w[j] >> (8*b));
}
static void ld_w64( uint64_t (&w)[4], uint8_t const * p ) {
  for( int j=0; j<4; j++ ) { uint64_t v = 0; for( int b=7; b>=0; b-- ) v = (v << 8) | p[8*j+b]; w[j] = v; }
}
static void st_w64( uint8_t * p, uint64_t const (&w)[4] ) {
  for( int j=0; j<4; j++ ) for( int b=0; b<8; b++ ) p[8*j+b] = (uint8_t)(w[j] >> (8*b));
}

/* 64 lanes of a wave as an array */
#define LANES 64
struct hv {
  fd_gpu_fe_t e[LANES];
  static hv mul( hv const & a, hv const & b ) { hv r; for( int l=0; l<LANES; l++ ) fd_fe_mul( r.e[l], a.e[l], b.e[l] ); return r; }
  static hv up( hv const & a, int d ) {
    hv r; for( int l=0; l<LANES; l++ ) { if( l >= d ) r.e[l] = a.e[l-d]; else fd_fe_set( r.e[l], 1 ); } return r;
  }
  static hv down( hv const & a, int d ) {
    hv r; for( int l=0; l<LANES; l++ ) { if( l + d < LANES ) r.e[l] = a.e[l+d]; else fd_fe_set( r.e[l], 1 ); } return r;
  }
  static hv last( hv const & a ) { hv r; for( int l=0; l<LANES; l++ ) r.e[l] = a.e[LANES-1]; return r; }
  static hv invert( hv const & a ) { hv r; for( int l=0; l<LANES; l++ ) fd_fe_invert( r.e[l], a.e[l] ); return r; }
};

extern "C" {

int const * h_sgn_comb( int * entries, int * entry_dw ) { *entries = FD_SGN_TAB_ENTRIES; *entry_dw = FD_SGN_TAB_ENTRY_DW; return fd_sgn_comb; }

/* out[32 i ..) = the encoding of [s_i]B, one inversion each */
void h_base_mul_enc( uint8_t * out, uint8_t const * s, unsigned long n ) {
  for( unsigned long i=0; i<n; i++ ) {
    uint32_t w[8], enc[8]; ld_words( w, s + 32*i );
    fd_sgn_p3_t P; fd_sgn_base_mul( P, w, (tabp)fd_sgn_comb );
    fd_gpu_fe_t zi; fd_fe_invert( zi, P.Z );
    fd_sgn_encode( enc, P.X, P.Y, zi );
    st_words( out + 32*i, enc );
  }
}

/* one wave of 64 lanes: lane l < nact with skip[l] == 0 encodes [s_l]B
   through the batched inversion; every other lane hands in 1 and gets 32
   zero bytes */
void h_base_mul_enc_wave( uint8_t * out, uint8_t const * s, int nact, uint8_t const * skip ) {
  static fd_sgn_p3_t P[LANES];
  hv z, zi;
  for( int l=0; l<LANES; l++ ) {
    bool on = l < nact && !skip[l];
    fd_fe_set( z.e[l], 1 );
    if( on ) { uint32_t w[8]; ld_words( w, s + 32*l ); fd_sgn_base_mul( P[l], w, (tabp)fd_sgn_comb ); z.e[l] = P[l].Z; }
  }
  fd_sgn_batch_invert( zi, z );
  for( int l=0; l<LANES; l++ ) {
    bool on = l < nact && !skip[l];
    uint32_t enc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if( on ) fd_sgn_encode( enc, P[l].X, P[l].Y, zi.e[l] );
    st_words( out + 32*l, enc );
  }
}

void h_sc_muladd( uint8_t * out, uint8_t const * k, uint8_t const * a, uint8_t const * r, unsigned long n ) {
  for( unsigned long i=0; i<n; i++ ) {
    uint64_t kw[4], aw[4], rw[4], s[4];
    ld_w64( kw, k + 32*i ); ld_w64( aw, a + 32*i ); ld_w64( rw, r + 32*i );
    fd_sgn_sc_muladd( s, kw, aw, rw );
    st_w64( out + 32*i, s );
  }
}

static void seed_words( uint64_t (&sw)[4], uint8_t const * seed ) {
  for( int j=0; j<4; j++ ) { uint64_t v = 0; for( int b=0; b<8; b++ ) v = (v << 8) | seed[8*j+b]; sw[j] = v; }
}

void h_public( uint8_t * pub, uint8_t const * seed ) {
  uint64_t sw[4], prefix[4]; uint32_t a[8], enc[8];
  seed_words( sw, seed );
  fd_sgn_expand( a, prefix, sw );
  fd_sgn_p3_t P; fd_sgn_base_mul( P, a, (tabp)fd_sgn_comb );
  fd_gpu_fe_t zi; fd_fe_invert( zi, P.Z );
  fd_sgn_encode( enc, P.X, P.Y, zi );
  st_words( pub, enc );
}

/* the kernel's chain for one signature: pub_in NULL derives the key (both
   encodings from one inversion, as fd_k_sign); pub_out (optional) = the key used */
void h_sign( uint8_t * sig, uint8_t * pub_out, uint8_t const * seed, uint8_t const * pub_in, uint8_t const * msg, uint32_t sz ) {
  uint64_t sw[4], prefix[4], r[4], S[4]; uint32_t a[8], rw[8], Aenc[8], Renc[8];
  seed_words( sw, seed );
  fd_sgn_expand( a, prefix, sw );
  fd_sgn_nonce( r, prefix, msg, sz );
  for( int k=0; k<8; k++ ) rw[k] = (uint32_t)( r[k>>1] >> (32*(k&1)) );
  fd_sgn_p3_t PA, PR;
  fd_fe_set( PA.X, 0 ); fd_fe_set( PA.Y, 1 ); fd_fe_set( PA.Z, 1 ); fd_fe_set( PA.T, 0 );
  if( !pub_in ) fd_sgn_base_mul( PA, a, (tabp)fd_sgn_comb );
  fd_sgn_base_mul( PR, rw, (tabp)fd_sgn_comb );
  fd_gpu_fe_t zz, zi, zai, zri;
  fd_fe_mul( zz, PA.Z, PR.Z );
  fd_fe_invert( zi, zz );
  fd_fe_mul2( zai, zi, PR.Z, zri, zi, PA.Z );
  fd_sgn_encode( Aenc, PA.X, PA.Y, zai );
  fd_sgn_encode( Renc, PR.X, PR.Y, zri );
  if( pub_in ) ld_words( Aenc, pub_in );
  fd_sgn_finish( S, Renc, Aenc, msg, sz, a, r );
  st_words( sig, Renc ); st_w64( sig + 32, S );
  if( pub_out ) st_words( pub_out, Aenc );
}

}

#ifdef SIGN_HARNESS_MAIN
static int fails = 0;
static void expect( char const * what, uint8_t const * got, uint8_t const * exp, unsigned long sz ) {
  if( memcmp( got, exp, sz ) ) { fails++; printf( "FAIL %s\n", what ); }
}
static void unhex( uint8_t * out, char const * h ) {
  for( unsigned long i=0; h[2*i]; i++ ) { unsigned v; sscanf( h + 2*i, "%2x", &v ); out[i] = (uint8_t)v; }
}

int main( void ) {
  /* edge scalars: 0, 1, 8, L-1, L, 2^252, every nibble 8, every nibble 0xF, 2^255-1 */
  static char const * L_hex = "edd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010";
  uint8_t s[9][32]; memset( s, 0, sizeof(s) );
  s[1][0] = 1; s[2][0] = 8;
  unhex( s[3], L_hex ); s[3][0]--;
  unhex( s[4], L_hex );
  s[5][31] = 0x10;
  memset( s[6], 0x88, 32 ); memset( s[7], 0xff, 32 ); memset( s[8], 0xff, 32 ); s[8][31] = 0x7f;
  uint8_t enc[9][32];
  h_base_mul_enc( &enc[0][0], &s[0][0], 9 );
  uint8_t ident[32] = { 1 }, base[32];
  unhex( base, "5866666666666666666666666666666666666666666666666666666666666666" );
  expect( "[0]B", enc[0], ident, 32 );
  expect( "[1]B", enc[1], base, 32 );
  expect( "[L]B", enc[4], ident, 32 );
  /* [L-1]B = -B: the same y, the other sign */
  base[31] ^= 0x80; expect( "[L-1]B", enc[3], base, 32 ); base[31] ^= 0x80;

  /* the batched inversion at wave sizes 1, 2, 63, 64 and with rejected lanes */
  static uint8_t ws[64][32], wave[64][32], lone[64][32], skip[64];
  for( int l=0; l<64; l++ ) for( int b=0; b<32; b++ ) ws[l][b] = (uint8_t)(37*l + 11*b + (l*b)%7 + 1);
  for( int l=0; l<9; l++ ) memcpy( ws[l], s[l], 32 );
  h_base_mul_enc( &lone[0][0], &ws[0][0], 64 );
  int const sizes[4] = { 1, 2, 63, 64 };
  for( int t=0; t<5; t++ ) {
    memset( skip, 0, sizeof(skip) );
    int nact = t < 4 ? sizes[t] : 64;
    if( t == 4 ) { skip[0] = 1; skip[31] = 1; skip[63] = 1; }
    h_base_mul_enc_wave( &wave[0][0], &ws[0][0], nact, skip );
    for( int l=0; l<64; l++ ) {
      static uint8_t const zero[32] = { 0 };
      expect( "wave inversion", wave[l], ( l < nact && !skip[l] ) ? lone[l] : zero, 32 );
    }
  }

  /* sc_muladd: all zero; k = r = L-1 with a = 2^255 - 8 -> (L-1)(a+1) mod L */
  uint8_t k[32], a[32], r[32], o[32], z32[32] = { 0 };
  memset( k, 0, 32 ); memset( a, 0, 32 ); memset( r, 0, 32 );
  h_sc_muladd( o, k, a, r, 1 );
  expect( "muladd zero", o, z32, 32 );
  memcpy( k, s[3], 32 ); memcpy( r, s[3], 32 ); memset( a, 0xff, 32 ); a[0] = 0xf8; a[31] = 0x7f;
  h_sc_muladd( o, k, a, r, 1 );
  {
    /* k = L-1 = -1, so o = -(a + 1) mod L: checked as 1 (a + 1) + o = 0 mod L */
    uint8_t one[32] = { 1 }, a1[32], chk[32];
    memcpy( a1, a, 32 ); a1[0] = 0xf9;                 /* a + 1 = 2^255 - 7 */
    h_sc_muladd( chk, one, a1, o, 1 );                 /* (a+1) + o mod L */
    expect( "muladd L-1", chk, z32, 32 );
  }

  /* RFC 8032 7.1 TEST 1 and TEST 2 through the whole chain */
  uint8_t seed[32], pub[32], sig[64], epub[32], esig[64], msg[1];
  unhex( seed, "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60" );
  unhex( epub, "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a" );
  unhex( esig, "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b" );
  h_sign( sig, pub, seed, NULL, NULL, 0 );
  expect( "RFC TEST 1 pub", pub, epub, 32 ); expect( "RFC TEST 1 sig", sig, esig, 64 );
  h_sign( sig, NULL, seed, epub, NULL, 0 );
  expect( "RFC TEST 1 sig (key given)", sig, esig, 64 );
  unhex( seed, "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb" );
  unhex( epub, "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c" );
  unhex( esig, "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00" );
  msg[0] = 0x72;
  h_sign( sig, pub, seed, NULL, msg, 1 );
  expect( "RFC TEST 2 pub", pub, epub, 32 ); expect( "RFC TEST 2 sig", sig, esig, 64 );
  h_public( pub, seed );
  expect( "RFC TEST 2 public", pub, epub, 32 );

  printf( fails ? "%d failures\n" : "ok\n", fails );
  return fails ? 1 : 0;
}
#endif
