#ifndef HEADER_fd_poh_core_h
#define HEADER_fd_poh_core_h

/* fd_poh_core.h -- the two SHA-256 bodies of the Proof-of-History chain
   (reference src/ballet/poh/fd_poh.c:3-24), specialised to their fixed
   message shapes and shared by the host routines (fd_poh_host.c) and the
   device kernel (fd_k_poh, one lane per entry).

     fd_poh_step: s <- SHA-256( s )        32-byte message, one compression
     fd_poh_mix : s <- SHA-256( s || m )   64-byte message, two compressions

   The state is eight host-order words between iterations; bytes are
   swapped only where a state is loaded from or stored to memory
   (fd_poh_load / fd_poh_store).  Both messages have a fixed length, so
   their padding is constant: in fd_poh_step the upper half of the block
   (W[8] = 0x80000000, W[9..14] = 0, W[15] = 256) is written as literals
   and folds into the unrolled schedule, and the second block of fd_poh_mix
   is padding only, so its 64 K[t]+W[t] sums are a table (fd_poh_kw2) and
   it has no schedule at all.

   static inline, C and C++, no libc, no memory besides the arguments. */

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FD_POH_CORE_FN static inline __host__ __device__ __attribute__((always_inline))
#else
#define FD_POH_CORE_FN static inline __attribute__((always_inline))
#endif

/* rotates as v_alignbit_b32, three-input xor and majority as one
   v_bitop3_b32 each (truth tables 0x96 and 0xE8, both symmetric in their
   inputs), Ch as a bit-field insert (the compiler's pick for the select
   form below) */
#if defined(__HIP_DEVICE_COMPILE__)
#define FD_POH_ROTR(x,n)   __builtin_amdgcn_alignbit( (x), (x), (uint32_t)(n) )
#define FD_POH_XOR3(x,y,z) __builtin_amdgcn_bitop3_b32( (x), (y), (z), 0x96 )
#define FD_POH_MAJ(x,y,z)  __builtin_amdgcn_bitop3_b32( (x), (y), (z), 0xE8 )
#else
#define FD_POH_ROTR(x,n)   ( ((x) >> (n)) | ((x) << (32-(n))) )
#define FD_POH_XOR3(x,y,z) ( (x) ^ (y) ^ (z) )
#define FD_POH_MAJ(x,y,z)  ( ((x) & (y)) | ((z) & ((x) | (y))) )
#endif
#define FD_POH_CH(x,y,z)   ( (z) ^ ( (x) & ( (y) ^ (z) ) ) )
#define FD_POH_BS0(x)      FD_POH_XOR3( FD_POH_ROTR(x, 2), FD_POH_ROTR(x,13), FD_POH_ROTR(x,22) )
#define FD_POH_BS1(x)      FD_POH_XOR3( FD_POH_ROTR(x, 6), FD_POH_ROTR(x,11), FD_POH_ROTR(x,25) )
#define FD_POH_SS0(x)      FD_POH_XOR3( FD_POH_ROTR(x, 7), FD_POH_ROTR(x,18), ((x) >>  3) )
#define FD_POH_SS1(x)      FD_POH_XOR3( FD_POH_ROTR(x,17), FD_POH_ROTR(x,19), ((x) >> 10) )

#define FD_POH_IV0 0x6a09e667U
#define FD_POH_IV1 0xbb67ae85U
#define FD_POH_IV2 0x3c6ef372U
#define FD_POH_IV3 0xa54ff53aU
#define FD_POH_IV4 0x510e527fU
#define FD_POH_IV5 0x9b05688cU
#define FD_POH_IV6 0x1f83d9abU
#define FD_POH_IV7 0x5be0cd19U

/* one round; the caller rotates the roles of a..h instead of the values */
#define FD_POH_RND(a,b,c,d,e,f,g,h,kw) do {                                     \
    uint32_t t1_ = (h) + FD_POH_BS1(e) + FD_POH_CH(e,f,g) + (kw);               \
    (d) += t1_;                                                                 \
    (h)  = t1_ + FD_POH_BS0(a) + FD_POH_MAJ(a,b,c);                             \
  } while(0)

/* schedule word t >= 16 in the 16-word rolling window */
#define FD_POH_SCHED(w,t) ( (w)[(t)&15] += FD_POH_SS1( (w)[((t)-2)&15] ) + (w)[((t)-7)&15] + FD_POH_SS0( (w)[((t)-15)&15] ) )

/* eight rounds t..t+7 with X(t') giving K[t']+W[t'] */
#define FD_POH_RND8(X,t)                      \
  FD_POH_RND(a,b,c,d,e,f,g,h,X((t)+0));       \
  FD_POH_RND(h,a,b,c,d,e,f,g,X((t)+1));       \
  FD_POH_RND(g,h,a,b,c,d,e,f,X((t)+2));       \
  FD_POH_RND(f,g,h,a,b,c,d,e,X((t)+3));       \
  FD_POH_RND(e,f,g,h,a,b,c,d,X((t)+4));       \
  FD_POH_RND(d,e,f,g,h,a,b,c,X((t)+5));       \
  FD_POH_RND(c,d,e,f,g,h,a,b,X((t)+6));       \
  FD_POH_RND(b,c,d,e,f,g,h,a,X((t)+7))

#define FD_POH_K_LIST \
  0x428a2f98U,0x71374491U,0xb5c0fbcfU,0xe9b5dba5U,0x3956c25bU,0x59f111f1U,0x923f82a4U,0xab1c5ed5U, \
  0xd807aa98U,0x12835b01U,0x243185beU,0x550c7dc3U,0x72be5d74U,0x80deb1feU,0x9bdc06a7U,0xc19bf174U, \
  0xe49b69c1U,0xefbe4786U,0x0fc19dc6U,0x240ca1ccU,0x2de92c6fU,0x4a7484aaU,0x5cb0a9dcU,0x76f988daU, \
  0x983e5152U,0xa831c66dU,0xb00327c8U,0xbf597fc7U,0xc6e00bf3U,0xd5a79147U,0x06ca6351U,0x14292967U, \
  0x27b70a85U,0x2e1b2138U,0x4d2c6dfcU,0x53380d13U,0x650a7354U,0x766a0abbU,0x81c2c92eU,0x92722c85U, \
  0xa2bfe8a1U,0xa81a664bU,0xc24b8b70U,0xc76c51a3U,0xd192e819U,0xd6990624U,0xf40e3585U,0x106aa070U, \
  0x19a4c116U,0x1e376c08U,0x2748774cU,0x34b0bcb5U,0x391c0cb3U,0x4ed8aa4aU,0x5b9cca4fU,0x682e6ff3U, \
  0x748f82eeU,0x78a5636fU,0x84c87814U,0x8cc70208U,0x90befffaU,0xa4506cebU,0xbef9a3f7U,0xc67178f2U

/* K[t]+W[t] of the block that is only the padding of a 64-byte message:
   W[0] = 0x80000000, W[1..14] = 0, W[15] = 512, W[16..63] by the schedule
   (tests/test_poh_host.py recomputes the table) */
#define FD_POH_KW2_LIST \
  0xc28a2f98U,0x71374491U,0xb5c0fbcfU,0xe9b5dba5U,0x3956c25bU,0x59f111f1U,0x923f82a4U,0xab1c5ed5U, \
  0xd807aa98U,0x12835b01U,0x243185beU,0x550c7dc3U,0x72be5d74U,0x80deb1feU,0x9bdc06a7U,0xc19bf374U, \
  0x649b69c1U,0xf0fe4786U,0x0fe1edc6U,0x240cf254U,0x4fe9346fU,0x6cc984beU,0x61b9411eU,0x16f988faU, \
  0xf2c65152U,0xa88e5a6dU,0xb019fc65U,0xb9d99ec7U,0x9a1231c3U,0xe70eeaa0U,0xfdb1232bU,0xc7353eb0U, \
  0x3069bad5U,0xcb976d5fU,0x5a0f118fU,0xdc1eeefdU,0x0a35b689U,0xde0b7a04U,0x58f4ca9dU,0xe15d5b16U, \
  0x007f3e86U,0x37088980U,0xa507ea32U,0x6fab9537U,0x17406110U,0x0d8cd6f1U,0xcdaa3b6dU,0xc0bbbe37U, \
  0x83613bdaU,0xdb48a363U,0x0b02e931U,0x6fd15ca7U,0x521afacaU,0x31338431U,0x6ed41a95U,0x6d437890U, \
  0xc39c91f2U,0x9eccabbdU,0xb5c9a0e6U,0x532fb63cU,0xd2c741c6U,0x07237ea3U,0xa4954b68U,0x4c191d76U

/* The tables are local constant arrays indexed by literals only: after
   unrolling every element is an immediate (on the device a 32-bit literal
   operand), and nothing is loaded. */

/* s += the 64 rounds of one block from working state s, w[0..15] the
   block's words (destroyed) */
FD_POH_CORE_FN void fd_poh_compress( uint32_t s[8], uint32_t w[16] ) {
  uint32_t const k[64] = { FD_POH_K_LIST };
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#define FD_POH_X0(t) ( k[t] + w[(t)&15] )
#define FD_POH_X1(t) ( k[t] + FD_POH_SCHED( w, t ) )
  FD_POH_RND8( FD_POH_X0,  0 ); FD_POH_RND8( FD_POH_X0,  8 );
  FD_POH_RND8( FD_POH_X1, 16 ); FD_POH_RND8( FD_POH_X1, 24 );
  FD_POH_RND8( FD_POH_X1, 32 ); FD_POH_RND8( FD_POH_X1, 40 );
  FD_POH_RND8( FD_POH_X1, 48 ); FD_POH_RND8( FD_POH_X1, 56 );
#undef FD_POH_X0
#undef FD_POH_X1
  s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

/* s <- SHA-256( s as 32 big-endian bytes ) */
FD_POH_CORE_FN void fd_poh_step( uint32_t s[8] ) {
  uint32_t w[16];
  w[0] = s[0]; w[1] = s[1]; w[2] = s[2]; w[3] = s[3]; w[4] = s[4]; w[5] = s[5]; w[6] = s[6]; w[7] = s[7];
  w[8] = 0x80000000U; w[9] = 0U; w[10] = 0U; w[11] = 0U; w[12] = 0U; w[13] = 0U; w[14] = 0U; w[15] = 256U;
  s[0] = FD_POH_IV0; s[1] = FD_POH_IV1; s[2] = FD_POH_IV2; s[3] = FD_POH_IV3;
  s[4] = FD_POH_IV4; s[5] = FD_POH_IV5; s[6] = FD_POH_IV6; s[7] = FD_POH_IV7;
  fd_poh_compress( s, w );
}

/* s <- SHA-256( s || m ), m as eight big-endian words */
FD_POH_CORE_FN void fd_poh_mix( uint32_t s[8], uint32_t const m[8] ) {
  uint32_t const kw[64] = { FD_POH_KW2_LIST };
  uint32_t w[16];
  w[0] = s[0]; w[1] = s[1]; w[2]  = s[2]; w[3]  = s[3]; w[4]  = s[4]; w[5]  = s[5]; w[6]  = s[6]; w[7]  = s[7];
  w[8] = m[0]; w[9] = m[1]; w[10] = m[2]; w[11] = m[3]; w[12] = m[4]; w[13] = m[5]; w[14] = m[6]; w[15] = m[7];
  s[0] = FD_POH_IV0; s[1] = FD_POH_IV1; s[2] = FD_POH_IV2; s[3] = FD_POH_IV3;
  s[4] = FD_POH_IV4; s[5] = FD_POH_IV5; s[6] = FD_POH_IV6; s[7] = FD_POH_IV7;
  fd_poh_compress( s, w );
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#define FD_POH_X2(t) ( kw[t] )
  FD_POH_RND8( FD_POH_X2,  0 ); FD_POH_RND8( FD_POH_X2,  8 );
  FD_POH_RND8( FD_POH_X2, 16 ); FD_POH_RND8( FD_POH_X2, 24 );
  FD_POH_RND8( FD_POH_X2, 32 ); FD_POH_RND8( FD_POH_X2, 40 );
  FD_POH_RND8( FD_POH_X2, 48 ); FD_POH_RND8( FD_POH_X2, 56 );
#undef FD_POH_X2
  s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

/* 32 big-endian bytes <-> eight host-order words, byte by byte: any
   alignment */
FD_POH_CORE_FN void fd_poh_load( uint32_t s[8], uint8_t const * p ) {
  for( int j=0; j<8; j++ )
    s[j] = ((uint32_t)p[4*j] << 24) | ((uint32_t)p[4*j+1] << 16) | ((uint32_t)p[4*j+2] << 8) | (uint32_t)p[4*j+3];
}
FD_POH_CORE_FN void fd_poh_store( uint8_t * p, uint32_t const s[8] ) {
  for( int j=0; j<8; j++ ) {
    p[4*j] = (uint8_t)(s[j] >> 24); p[4*j+1] = (uint8_t)(s[j] >> 16); p[4*j+2] = (uint8_t)(s[j] >> 8); p[4*j+3] = (uint8_t)s[j];
  }
}

#endif /* HEADER_fd_poh_core_h */
