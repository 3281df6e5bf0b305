/* fd_ed25519_gpu_sign.h -- the arithmetic core of batch Ed25519 signing
   and key derivation (RFC 8032 5.1.5 / 5.1.6), one lane per signature.

   Everything here is __host__ __device__ (FD_DEV): the kernels of
   fd_ed25519_gpu_sign_kernels.hip run it on gfx950, and
   tests/sign_host_harness.cpp compiles the same functions for the CPU,
   where tests/test_sign_host.py holds them against a big-integer model
   and the oracle's signer.

   Secrets are the seed, az = SHA-512(seed), the clamped scalar a, the
   nonce r and every digit of a and r.  No branch and no memory address in
   this file depends on one: table lookups read all eight candidates of a
   comb position and keep one with lane masks (fd_sel), negation is a
   select, a zero digit is added like any other (the identity in cached
   form), and the scalar arithmetic is straight-line.  What does branch is
   public: message lengths, lane indices, descriptor bounds. */

#ifndef FD_ED25519_GPU_SIGN_CORE_H
#define FD_ED25519_GPU_SIGN_CORE_H

#include "fd_ed25519_gpu_fe.h"
#include "fd_ed25519_gpu_sha512.h"
#include "fd_ed25519_tables.h"

/* ---- SHA-512 of PRE prefix bytes || M ---------------------------------
   The prefix (PRE = 32: a seed, or az[32..64); PRE = 64: R || A) comes
   from registers as big-endian message words; message bytes come from
   memory at any alignment.  Streaming semantics (padding byte, bit count)
   of FIPS 180-4 5.1.2. */

__host__ __device__ constexpr uint64_t fd_sgn_iv[8] = {
  0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
  0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };

#if !defined(__HIP_DEVICE_COMPILE__)
/* the host build's compression (fd_sha512_compress is built from gfx950
   instructions): FIPS 180-4 6.4.2 as written */
static uint64_t const fd_sgn_k[80] = {
  0x428a2f98d728ae22ULL,0x7137449123ef65cdULL,0xb5c0fbcfec4d3b2fULL,0xe9b5dba58189dbbcULL,0x3956c25bf348b538ULL,
  0x59f111f1b605d019ULL,0x923f82a4af194f9bULL,0xab1c5ed5da6d8118ULL,0xd807aa98a3030242ULL,0x12835b0145706fbeULL,
  0x243185be4ee4b28cULL,0x550c7dc3d5ffb4e2ULL,0x72be5d74f27b896fULL,0x80deb1fe3b1696b1ULL,0x9bdc06a725c71235ULL,
  0xc19bf174cf692694ULL,0xe49b69c19ef14ad2ULL,0xefbe4786384f25e3ULL,0x0fc19dc68b8cd5b5ULL,0x240ca1cc77ac9c65ULL,
  0x2de92c6f592b0275ULL,0x4a7484aa6ea6e483ULL,0x5cb0a9dcbd41fbd4ULL,0x76f988da831153b5ULL,0x983e5152ee66dfabULL,
  0xa831c66d2db43210ULL,0xb00327c898fb213fULL,0xbf597fc7beef0ee4ULL,0xc6e00bf33da88fc2ULL,0xd5a79147930aa725ULL,
  0x06ca6351e003826fULL,0x142929670a0e6e70ULL,0x27b70a8546d22ffcULL,0x2e1b21385c26c926ULL,0x4d2c6dfc5ac42aedULL,
  0x53380d139d95b3dfULL,0x650a73548baf63deULL,0x766a0abb3c77b2a8ULL,0x81c2c92e47edaee6ULL,0x92722c851482353bULL,
  0xa2bfe8a14cf10364ULL,0xa81a664bbc423001ULL,0xc24b8b70d0f89791ULL,0xc76c51a30654be30ULL,0xd192e819d6ef5218ULL,
  0xd69906245565a910ULL,0xf40e35855771202aULL,0x106aa07032bbd1b8ULL,0x19a4c116b8d2d0c8ULL,0x1e376c085141ab53ULL,
  0x2748774cdf8eeb99ULL,0x34b0bcb5e19b48a8ULL,0x391c0cb3c5c95a63ULL,0x4ed8aa4ae3418acbULL,0x5b9cca4f7763e373ULL,
  0x682e6ff3d6b2b8a3ULL,0x748f82ee5defb2fcULL,0x78a5636f43172f60ULL,0x84c87814a1f0ab72ULL,0x8cc702081a6439ecULL,
  0x90befffa23631e28ULL,0xa4506cebde82bde9ULL,0xbef9a3f7b2c67915ULL,0xc67178f2e372532bULL,0xca273eceea26619cULL,
  0xd186b8c721c0c207ULL,0xeada7dd6cde0eb1eULL,0xf57d4f7fee6ed178ULL,0x06f067aa72176fbaULL,0x0a637dc5a2c898a6ULL,
  0x113f9804bef90daeULL,0x1b710b35131c471bULL,0x28db77f523047d84ULL,0x32caab7b40c72493ULL,0x3c9ebe0a15c9bebcULL,
  0x431d67c49c100d4cULL,0x4cc5d4becb3e42b6ULL,0x597f299cfc657e2aULL,0x5fcb6fab3ad6faecULL,0x6c44198c4a475817ULL
};
static inline uint64_t fd_sgn_ror( uint64_t x, int n ) { return (x >> n) | (x << (64 - n)); }
static inline void fd_sgn_compress_host( uint64_t (&st)[8], uint64_t const (&blk)[16] ) {
  uint64_t w[80];
  for( int t=0; t<16; t++ ) w[t] = blk[t];
  for( int t=16; t<80; t++ ) {
    uint64_t s0 = fd_sgn_ror( w[t-15], 1 ) ^ fd_sgn_ror( w[t-15], 8 ) ^ (w[t-15] >> 7);
    uint64_t s1 = fd_sgn_ror( w[t-2], 19 ) ^ fd_sgn_ror( w[t-2], 61 ) ^ (w[t-2] >> 6);
    w[t] = w[t-16] + s0 + w[t-7] + s1;
  }
  uint64_t a=st[0],b=st[1],c=st[2],d=st[3],e=st[4],f=st[5],g=st[6],h=st[7];
  for( int t=0; t<80; t++ ) {
    uint64_t t1 = h + (fd_sgn_ror( e, 14 ) ^ fd_sgn_ror( e, 18 ) ^ fd_sgn_ror( e, 41 )) + ((e & f) ^ (~e & g)) + fd_sgn_k[t] + w[t];
    uint64_t t2 = (fd_sgn_ror( a, 28 ) ^ fd_sgn_ror( a, 34 ) ^ fd_sgn_ror( a, 39 )) + ((a & b) ^ (a & c) ^ (b & c));
    h=g; g=f; f=e; e=d+t1; d=c; c=b; b=a; a=t1+t2;
  }
  st[0]+=a; st[1]+=b; st[2]+=c; st[3]+=d; st[4]+=e; st[5]+=f; st[6]+=g; st[7]+=h;
}
#endif

FD_DEV void fd_sgn_compress( uint64_t (&st)[8], uint64_t (&w)[16] ) {
#if defined(__HIP_DEVICE_COMPILE__)
  fd_sha512_compress( st, w );
#else
  fd_sgn_compress_host( st, w );
#endif
}

/* message bytes [off, off+8) as a big-endian word; bytes at or past sz
   read as zero.  A word wholly inside the message is one unaligned 8-byte
   fetch (the batch blob is readable 16 bytes past its end, as the verify
   path's loaders assume); the word the message ends in is read bytewise. */
FD_DEV uint64_t fd_sgn_msg_word( uint8_t const * M, uint32_t off, uint32_t sz ) {
  uint64_t v = 0UL;
  if( (uint64_t)off + 8UL <= (uint64_t)sz ) {
#if defined(__HIP_DEVICE_COMPILE__)
    v = fd_bswap64( fd_ld_u64_unaligned( M + off ) );
#else
    for( int j=0; j<8; j++ ) v = (v << 8) | (uint64_t)M[off + (uint32_t)j];
#endif
  } else {
    for( uint32_t j=0; j<8u; j++ ) {
      uint64_t b = ( off + j < sz ) ? (uint64_t)M[off + j] : 0UL;
      v = (v << 8) | b;
    }
  }
  return v;
}

/* dig = SHA-512( prefix(PRE bytes, words pw[0 .. PRE/8)) || M[0, sz) ) as
   the state words (word i = digest bytes 8i..8i+7 big endian).  One code
   instance of the compression per call site: block 0's prefix words are
   selected, not branched to. */
template<int PRE>
FD_DEV void fd_sgn_sha512( uint64_t (&st)[8], uint64_t const (&pw)[8], uint8_t const * M, uint32_t sz ) {
  static_assert( PRE == 32 || PRE == 64, "prefix is 32 or 64 bytes" );
#pragma unroll
  for( int i=0; i<8; i++ ) st[i] = fd_sgn_iv[i];
  uint64_t L = (uint64_t)PRE + (uint64_t)sz;
  uint32_t nblk = (uint32_t)((L + 17UL + 127UL) >> 7);
  for( uint32_t b=0; b<nblk; b++ ) {
    uint64_t w[16];
#pragma unroll
    for( int i=0; i<16; i++ ) {
      int64_t mp = (int64_t)b*128L + 8L*i - PRE;     /* message offset of this word's first byte */
      uint64_t v = 0UL;
      if( mp >= 0L && mp < (int64_t)sz ) v = fd_sgn_msg_word( M, (uint32_t)mp, sz );
      int64_t rem = (int64_t)sz - mp;                /* 0..7: the padding byte lies in this word */
      if( rem >= 0L && rem < 8L ) v |= 0x80UL << (56 - 8*(int)rem);
      if( i < PRE/8 ) v = b ? v : pw[i];
      if( i == 15 ) v = ( b == nblk-1u ) ? (L << 3) : v;
      w[i] = v;
    }
    fd_sgn_compress( st, w );
  }
}

/* the digest as little-endian 64-bit words (what fd_sc_reduce takes) */
FD_DEV void fd_sgn_dig_le( uint64_t (&le)[8], uint64_t const (&st)[8] ) {
#pragma unroll
  for( int i=0; i<8; i++ ) le[i] = __builtin_bswap64( st[i] );
}

/* ---- fixed-base multiplication ---------------------------------------- */

typedef struct { fd_gpu_fe_t X, Y, Z, T; } fd_sgn_p3_t;

#define FD_SGN_COMB_DW   30                  /* dwords per comb entry: y+x | y-x | 2dxy */
#define FD_SGN_COMB_ENTS 513                 /* 64 positions x 8 multiples + 16^64 B */
#define FD_SGN_COMB_DWS  (FD_SGN_COMB_DW*FD_SGN_COMB_ENTS)

/* r = p + e, e in cached affine form (y+x, y-x, 2dxy); the ref10 madd
   formulas (add-2008-hwcd-3 with Z2 = 1), then p1p1 -> p3.  Operand
   ranges: products leave |limb| <= 2^25 + 2^11; sums of two, and 2Z +- C,
   stay below 2^26.6, inside what fd_fe_mul's 19 g and 2 f pre-scales hold
   in 32 bits. */
FD_DEV void fd_sgn_madd( fd_sgn_p3_t & p, fd_gpu_fe_t const & ypx, fd_gpu_fe_t const & ymx, fd_gpu_fe_t const & xy2d ) {
  fd_gpu_fe_t a, b, c, d, e, f, g, h;
  fd_fe_add( a, p.Y, p.X );
  fd_fe_sub( b, p.Y, p.X );
  fd_fe_mul2( a, a, ypx, b, b, ymx );        /* A = (Y+X)(y+x), B = (Y-X)(y-x) */
  fd_fe_mul( c, p.T, xy2d );                 /* C = T 2dxy */
  fd_fe_add( d, p.Z, p.Z );                  /* D = 2Z */
  fd_fe_sub( e, a, b );                      /* E = A - B */
  fd_fe_add( h, a, b );                      /* H = A + B */
  fd_fe_add( g, d, c );                      /* G = D + C */
  fd_fe_sub( f, d, c );                      /* F = D - C */
  fd_fe_mul2( p.X, f, e, p.Y, g, h );        /* X = E F, Y = H G (the wider sums as first factors) */
  fd_fe_mul2( p.Z, g, f, p.T, h, e );        /* Z = G F, T = E H */
}

/* the entry |d| 16^i B (the identity for d = 0), negated for d < 0, kept
   out of all eight candidates by masks.  TP: pointer to the table (LDS on
   the device, memory on the host). */
template<typename TP>
FD_DEV void fd_sgn_lookup( fd_gpu_fe_t & ypx, fd_gpu_fe_t & ymx, fd_gpu_fe_t & xy2d, TP row, int32_t d ) {
  uint32_t neg = (uint32_t)(d >> 31);
  uint32_t ab  = ((uint32_t)d ^ neg) - neg;
  uint32_t e[FD_SGN_COMB_DW];
#pragma unroll
  for( int k=0; k<FD_SGN_COMB_DW; k++ ) e[k] = ( k == 0 || k == 10 ) ? 1u : 0u;     /* (1, 1, 0) */
#pragma unroll
  for( int j=1; j<=8; j++ ) {
    uint32_t m = (uint32_t)((int32_t)((ab ^ (uint32_t)j) - 1u) >> 31);               /* ab == j */
#pragma unroll
    for( int k=0; k<FD_SGN_COMB_DW; k++ ) e[k] = fd_sel( m, (uint32_t)row[(j-1)*FD_SGN_COMB_DW + k], e[k] );
  }
#pragma unroll
  for( int k=0; k<10; k++ ) {
    ypx.v[k]  = (int32_t)fd_sel( neg, e[10+k], e[k] );
    ymx.v[k]  = (int32_t)fd_sel( neg, e[k], e[10+k] );
    xy2d.v[k] = (int32_t)fd_sel( neg, 0u - e[20+k], e[20+k] );
  }
}

/* p = [s]B for any 256-bit s (8 little-endian words).  Signed radix-16
   digits, low to high: d = nibble + carry, carry = (d + 8) >> 4,
   d -= 16 carry, so every digit is in [-8, 7] and the carry out of digit
   63 (0 or 1) takes the table's last entry, 16^64 B.  65 additions, no
   doublings, none skipped. */
template<typename TP>
FD_DEV void fd_sgn_base_mul( fd_sgn_p3_t & p, uint32_t const (&s)[8], TP tab ) {
  uint32_t w[8];
#pragma unroll
  for( int i=0; i<8; i++ ) w[i] = s[i];
  fd_fe_set( p.X, 0 ); fd_fe_set( p.Y, 1 ); fd_fe_set( p.Z, 1 ); fd_fe_set( p.T, 0 );
  int32_t carry = 0;
#pragma unroll 1
  for( int i=0; i<64; i++ ) {
    int32_t d = (int32_t)(w[0] & 15u) + carry;
    carry = (d + 8) >> 4;
    d -= carry << 4;
#pragma unroll
    for( int k=0; k<7; k++ ) w[k] = (w[k] >> 4) | (w[k+1] << 28);
    w[7] >>= 4;
    fd_gpu_fe_t ypx, ymx, xy2d;
    fd_sgn_lookup( ypx, ymx, xy2d, tab + i*8*FD_SGN_COMB_DW, d );
    fd_sgn_madd( p, ypx, ymx, xy2d );
  }
  {
    /* the last carry: 16^64 B or the identity */
    uint32_t m = 0u - (uint32_t)carry;
    fd_gpu_fe_t ypx, ymx, xy2d;
#pragma unroll
    for( int k=0; k<10; k++ ) {
      ypx.v[k]  = (int32_t)fd_sel( m, (uint32_t)tab[512*FD_SGN_COMB_DW + k],      k == 0 ? 1u : 0u );
      ymx.v[k]  = (int32_t)fd_sel( m, (uint32_t)tab[512*FD_SGN_COMB_DW + 10 + k], k == 0 ? 1u : 0u );
      xy2d.v[k] = (int32_t)fd_sel( m, (uint32_t)tab[512*FD_SGN_COMB_DW + 20 + k], 0u );
    }
    fd_sgn_madd( p, ypx, ymx, xy2d );
  }
}

/* ---- point encoding ---------------------------------------------------- */

/* (X zinv, Y zinv) as the 32-byte encoding: y, with the sign of x in bit 255 */
FD_DEV void fd_sgn_encode( uint32_t (&out)[8], fd_gpu_fe_t const & X, fd_gpu_fe_t const & Y, fd_gpu_fe_t const & zinv ) {
  fd_gpu_fe_t x, y;
  fd_fe_mul2( x, X, zinv, y, Y, zinv );
  fd_fe_tobytes32( out, y );
  out[7] |= (uint32_t)fd_fe_isnegative( x ) << 31;
}

/* Montgomery's trick over the lanes of a wave.  V is a vector of lanes:
   the device's holds this lane's element and moves data with wave
   shuffles, the host model's (tests/sign_host_harness.cpp) holds all 64 in
   an array.  V provides
     V::mul( a, b )      lane-wise product
     V::up( a, d )       lane l takes lane l-d's element, lanes < d take 1
     V::down( a, d )     lane l takes lane l+d's element, lanes >= 64-d take 1
     V::last( a )        every lane takes lane 63's element
     V::invert( a )      lane-wise fd_fe_invert
   Inclusive prefix and suffix products by doubling (6 + 6 products), ONE
   inversion of the wave's total, then zinv[l] = total^-1 * prefix[l-1] *
   suffix[l+1].  A lane with nothing to invert (past n, or its descriptor
   rejected) hands in the field element 1. */
template<typename V>
FD_DEV void fd_sgn_batch_invert( V & zinv, V const & z ) {
  V p = z, s = z;
#pragma unroll 1
  for( int d=1; d<64; d<<=1 ) {
    V t = V::up( p, d );
    V u = V::down( s, d );
    p = V::mul( p, t );
    s = V::mul( s, u );
  }
  V inv = V::invert( V::last( p ) );
  zinv = V::mul( V::mul( inv, V::up( p, 1 ) ), V::down( s, 1 ) );
}

/* ---- S = (k a + r) mod L ---------------------------------------------- */

/* 21-bit limbs as fd_sc_reduce (ref10's sc_muladd schedule): the 23-limb
   product plus r, then the same folds of limbs 23..12 by
   2^252 = -27742317777372353535851937790883648493 (mod L).  k, r < L and
   a < 2^255 (clamped, not reduced); inputs and the canonical result as
   little-endian 64-bit words.  Straight-line. */
#define FD_SGN_FOLD(k) do { s[(k)-12] += s[k]*666643; s[(k)-11] += s[k]*470296; s[(k)-10] += s[k]*654183; \
                            s[(k)-9]  -= s[k]*997805; s[(k)-8]  += s[k]*136657; s[(k)-7]  -= s[k]*683901; s[k] = 0; } while(0)
#define FD_SGN_CR(k) do { int64_t c_ = (s[k] + (1LL<<20)) >> 21; s[(k)+1] += c_; s[k] -= (int64_t)((uint64_t)c_ << 21); } while(0)
#define FD_SGN_CF(k) do { int64_t c_ = s[k] >> 21;               s[(k)+1] += c_; s[k] -= (int64_t)((uint64_t)c_ << 21); } while(0)

FD_DEV void fd_sgn_limbs21( int64_t (&l)[12], uint64_t const (&in)[4] ) {
  uint64_t const m = (1UL<<21)-1UL;
#pragma unroll
  for( int i=0; i<11; i++ ) {
    int bit = 21*i, wd = bit>>6, sh = bit&63;
    uint64_t v = in[wd] >> sh;
    if( sh > 43 && wd+1 < 4 ) v |= in[wd+1] << (64-sh);
    l[i] = (int64_t)(v & m);
  }
  l[11] = (int64_t)(in[3] >> 39);            /* bits 231..255 */
}

FD_DEV void fd_sgn_sc_muladd( uint64_t (&out)[4], uint64_t const (&k)[4], uint64_t const (&a)[4], uint64_t const (&r)[4] ) {
  int64_t x[12], y[12], c[12], s[24];
  fd_sgn_limbs21( x, k ); fd_sgn_limbs21( y, a ); fd_sgn_limbs21( c, r );
#pragma unroll
  for( int i=0; i<24; i++ ) s[i] = i < 12 ? c[i] : 0L;
#pragma unroll
  for( int i=0; i<12; i++ )
#pragma unroll
    for( int j=0; j<12; j++ ) s[i+j] += x[i]*y[j];

  FD_SGN_CR(0); FD_SGN_CR(2); FD_SGN_CR(4); FD_SGN_CR(6); FD_SGN_CR(8); FD_SGN_CR(10);
  FD_SGN_CR(12); FD_SGN_CR(14); FD_SGN_CR(16); FD_SGN_CR(18); FD_SGN_CR(20); FD_SGN_CR(22);
  FD_SGN_CR(1); FD_SGN_CR(3); FD_SGN_CR(5); FD_SGN_CR(7); FD_SGN_CR(9); FD_SGN_CR(11);
  FD_SGN_CR(13); FD_SGN_CR(15); FD_SGN_CR(17); FD_SGN_CR(19); FD_SGN_CR(21);

#pragma unroll
  for( int i=23; i>=18; i-- ) FD_SGN_FOLD(i);
  FD_SGN_CR(6); FD_SGN_CR(8); FD_SGN_CR(10); FD_SGN_CR(12); FD_SGN_CR(14); FD_SGN_CR(16);
  FD_SGN_CR(7); FD_SGN_CR(9); FD_SGN_CR(11); FD_SGN_CR(13); FD_SGN_CR(15);
#pragma unroll
  for( int i=17; i>=12; i-- ) FD_SGN_FOLD(i);
  FD_SGN_CR(0); FD_SGN_CR(2); FD_SGN_CR(4); FD_SGN_CR(6); FD_SGN_CR(8); FD_SGN_CR(10);
  FD_SGN_CR(1); FD_SGN_CR(3); FD_SGN_CR(5); FD_SGN_CR(7); FD_SGN_CR(9); FD_SGN_CR(11);
  FD_SGN_FOLD(12);
#pragma unroll
  for( int i=0; i<12; i++ ) FD_SGN_CF(i);
  FD_SGN_FOLD(12);
#pragma unroll
  for( int i=0; i<11; i++ ) FD_SGN_CF(i);

  uint64_t u[12];
#pragma unroll
  for( int i=0; i<12; i++ ) u[i] = (uint64_t)s[i];
  out[0] = (u[0]    ) | (u[1] <<21) | (u[2] <<42) | (u[3] <<63);
  out[1] = (u[3] >>1) | (u[4] <<20) | (u[5] <<41) | (u[6] <<62);
  out[2] = (u[6] >>2) | (u[7] <<19) | (u[8] <<40) | (u[9] <<61);
  out[3] = (u[9] >>3) | (u[10]<<18) | (u[11]<<39);
}

#undef FD_SGN_FOLD
#undef FD_SGN_CR
#undef FD_SGN_CF

/* ---- one signature ----------------------------------------------------- */

/* a (clamped, 8 little-endian words) and the nonce prefix az[32..64) (4
   big-endian message words) from the seed's 32 bytes (4 big-endian words) */
FD_DEV void fd_sgn_expand( uint32_t (&a)[8], uint64_t (&prefix)[4], uint64_t const (&seed)[4] ) {
  uint64_t pw[8], st[8];
#pragma unroll
  for( int i=0; i<8; i++ ) pw[i] = i < 4 ? seed[i] : 0UL;
  fd_sgn_sha512<32>( st, pw, (uint8_t const *)0, 0u );
#pragma unroll
  for( int i=0; i<4; i++ ) {
    uint64_t le = __builtin_bswap64( st[i] );
    a[2*i] = (uint32_t)le; a[2*i+1] = (uint32_t)(le >> 32);
    prefix[i] = st[4+i];
  }
  a[0] &= ~7u; a[7] &= 0x3fffffffu; a[7] |= 0x40000000u;
#pragma unroll
  for( int i=0; i<8; i++ ) st[i] = 0UL;
}

/* r = SHA-512( prefix || M ) mod L */
FD_DEV void fd_sgn_nonce( uint64_t (&r)[4], uint64_t const (&prefix)[4], uint8_t const * M, uint32_t sz ) {
  uint64_t pw[8], st[8], le[8];
#pragma unroll
  for( int i=0; i<8; i++ ) pw[i] = i < 4 ? prefix[i] : 0UL;
  fd_sgn_sha512<32>( st, pw, M, sz );
  fd_sgn_dig_le( le, st );
  fd_sc_reduce( r, le );
}

/* S = (SHA-512( R || A || M ) mod L) a + r mod L; R and A as 8
   little-endian words each */
FD_DEV void fd_sgn_finish( uint64_t (&S)[4], uint32_t const (&R)[8], uint32_t const (&A)[8], uint8_t const * M, uint32_t sz,
                           uint32_t const (&a)[8], uint64_t const (&r)[4] ) {
  uint64_t pw[8], st[8], le[8], k[4], aw[4];
#pragma unroll
  for( int i=0; i<4; i++ ) {
    pw[i]   = __builtin_bswap64( ((uint64_t)R[2*i+1] << 32) | R[2*i] );
    pw[4+i] = __builtin_bswap64( ((uint64_t)A[2*i+1] << 32) | A[2*i] );
    aw[i]   = ((uint64_t)a[2*i+1] << 32) | a[2*i];
  }
  fd_sgn_sha512<64>( st, pw, M, sz );
  fd_sgn_dig_le( le, st );
  fd_sc_reduce( k, le );
  fd_sgn_sc_muladd( S, k, aw, r );
}

#endif /* FD_ED25519_GPU_SIGN_CORE_H */
