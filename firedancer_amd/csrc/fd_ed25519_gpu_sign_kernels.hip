/* fd_ed25519_gpu_sign_kernels.hip -- batch Ed25519 signing and key
   derivation for gfx950, one lane per signature.

   A translation unit of its own: the verify kernels
   (fd_ed25519_gpu_kernels.hip) and their build id do not move when this
   file does.  It includes the verify path's field, SHA-512 and scalar
   headers unchanged; the arithmetic is fd_ed25519_gpu_sign_core.h (also
   compiled for the CPU by tests/sign_host_harness.cpp).

   Layout of a block: 256 lanes = 256 signatures.  The comb
   (fd_ed25519_sign_tables.h: 64 positions x 8 multiples + 16^64 B, 30
   limbs each, 61,560 bytes) sits in HBM with the code object and is staged
   into LDS once per block; two blocks fit a CU's 160 KiB.  Every lane of a
   wave reads the same eight entries of a position (the address depends on
   the position alone, so the reads broadcast and never conflict) and keeps
   one by masks.  az, a and r live in registers only: no global scratch
   holds a secret, so there is nothing to wipe at exit. */

#include <hip/hip_runtime.h>
#include <stdint.h>

#define FD_SGN_TAB_QUAL __device__ __attribute__((aligned(16)))
#include "fd_ed25519_gpu_sign_core.h"
#include "fd_ed25519_sign_tables.h"
#include "fd_ed25519_gpu_sign_private.h"

static_assert( FD_SGN_TAB_ENTRIES == FD_SGN_COMB_ENTS && FD_SGN_TAB_ENTRY_DW == FD_SGN_COMB_DW, "comb geometry" );

#define FD_SGN_WG 256

typedef __attribute__((address_space(3))) int32_t const fd_sgn_lds_i32;

/* the comb into this block's LDS (8-byte copies: 7,695 per block) */
static __device__ __forceinline__ void fd_sgn_stage_comb( int32_t * lt ) {
  static_assert( FD_SGN_COMB_DWS % 2 == 0, "staged in dword pairs" );
  uint2 const * src = (uint2 const *)fd_sgn_comb;
  uint2 *       dst = (uint2 *)lt;
  for( uint32_t i=threadIdx.x; i<FD_SGN_COMB_DWS/2; i+=FD_SGN_WG ) dst[i] = src[i];
  __syncthreads();
}

/* this lane's element of a wave-wide vector (fd_sgn_batch_invert) */
struct fd_sgn_wave_v {
  fd_gpu_fe_t e;
  static __device__ __forceinline__ fd_sgn_wave_v mul( fd_sgn_wave_v const & a, fd_sgn_wave_v const & b ) {
    fd_sgn_wave_v r; fd_fe_mul( r.e, a.e, b.e ); return r;
  }
  static __device__ __forceinline__ fd_sgn_wave_v up( fd_sgn_wave_v const & a, int d ) {
    fd_sgn_wave_v r; bool in = (int)(threadIdx.x & 63u) >= d;
#pragma unroll
    for( int k=0; k<10; k++ ) { int32_t t = __shfl_up( a.e.v[k], (unsigned)d, 64 ); r.e.v[k] = in ? t : ( k ? 0 : 1 ); }
    return r;
  }
  static __device__ __forceinline__ fd_sgn_wave_v down( fd_sgn_wave_v const & a, int d ) {
    fd_sgn_wave_v r; bool in = (int)(threadIdx.x & 63u) + d < 64;
#pragma unroll
    for( int k=0; k<10; k++ ) { int32_t t = __shfl_down( a.e.v[k], (unsigned)d, 64 ); r.e.v[k] = in ? t : ( k ? 0 : 1 ); }
    return r;
  }
  static __device__ __forceinline__ fd_sgn_wave_v last( fd_sgn_wave_v const & a ) {
    fd_sgn_wave_v r;
#pragma unroll
    for( int k=0; k<10; k++ ) r.e.v[k] = __shfl( a.e.v[k], 63, 64 );
    return r;
  }
  static __device__ __forceinline__ fd_sgn_wave_v invert( fd_sgn_wave_v const & a ) {
    fd_sgn_wave_v r; fd_fe_invert( r.e, a.e ); return r;
  }
};

/* zinv = 1/z.  BATCH: every lane of the wave must call (lanes with nothing
   to invert pass z = 1). */
template<int BATCH>
static __device__ __forceinline__ void fd_sgn_invert( fd_gpu_fe_t & zinv, fd_gpu_fe_t const & z ) {
  if constexpr( BATCH ) {
    fd_sgn_wave_v in, out; in.e = z;
    fd_sgn_batch_invert( out, in );
    zinv = out.e;
  } else {
    fd_fe_invert( zinv, z );
  }
}

/* 32 bytes at any alignment as 4 big-endian message words */
static __device__ __forceinline__ void fd_sgn_ld32_be( uint64_t (&w)[4], uint8_t const * p ) {
#pragma unroll
  for( int i=0; i<4; i++ ) w[i] = fd_bswap64( fd_ld_u64_unaligned( p + 8*i ) );
}

template<int BATCH>
static __device__ __forceinline__ void
fd_sign_body( uint64_t n, uint8_t const * __restrict__ blob, uint64_t blob_sz, fd_ed25519_gpu_sign_desc_t const * __restrict__ sdesc,
              uint8_t * __restrict__ sig_out, uint8_t * __restrict__ pub_out, int32_t * __restrict__ status, fd_sgn_lds_i32 * tab ) {
  uint64_t const i = (uint64_t)blockIdx.x * FD_SGN_WG + threadIdx.x;
  bool const live = i < n;
  fd_ed25519_gpu_sign_desc_t d = { 0u, 0u, 0u, 0u };
  if( live ) d = sdesc[i];
  bool const derive = d.pub_off == FD_ED25519_GPU_SIGN_DERIVE;
  /* a descriptor outside the blob is never dereferenced (64-bit sums: no offset wraps) */
  bool const ok = live && (uint64_t)d.seed_off + 32UL <= blob_sz && (uint64_t)d.msg_off + (uint64_t)d.msg_sz <= blob_sz
               && ( derive || (uint64_t)d.pub_off + 32UL <= blob_sz );
  uint8_t const * M  = blob + ( ok ? d.msg_off : 0u );
  uint32_t const  sz = ok ? d.msg_sz : 0u;

  uint64_t seed[4] = { 0UL, 0UL, 0UL, 0UL };
  if( ok ) fd_sgn_ld32_be( seed, blob + d.seed_off );
  uint32_t a[8]; uint64_t prefix[4], r[4];
  fd_sgn_expand( a, prefix, seed );
  fd_sgn_nonce( r, prefix, M, sz );

  /* A = [a]B only in waves where some lane derives its key (wave-uniform:
     which descriptors derive is public), R = [r]B always: one instance of
     the comb loop */
  fd_sgn_p3_t PA, PR;
  fd_fe_set( PA.X, 0 ); fd_fe_set( PA.Y, 1 ); fd_fe_set( PA.Z, 1 ); fd_fe_set( PA.T, 0 );
  PR = PA;
  int const any_derive = __any( ok && derive );
#pragma unroll 1
  for( int pass = any_derive ? 0 : 1; pass < 2; pass++ ) {
    uint32_t s[8];
#pragma unroll
    for( int k=0; k<8; k++ ) s[k] = pass ? (uint32_t)( r[k>>1] >> (32*(k&1)) ) : a[k];
    fd_sgn_p3_t P;
    fd_sgn_base_mul( P, s, tab );
    if( pass ) PR = P; else PA = P;
  }

  /* both encodings from one inversion: 1/(ZA ZR), times ZR, times ZA */
  fd_gpu_fe_t zz, zi, zai, zri, one;
  fd_fe_set( one, 1 );
  fd_fe_mul( zz, PA.Z, PR.Z );
#pragma unroll
  for( int k=0; k<10; k++ ) zz.v[k] = ok ? zz.v[k] : one.v[k];
  fd_sgn_invert<BATCH>( zi, zz );
  fd_fe_mul2( zai, zi, PR.Z, zri, zi, PA.Z );
  uint32_t Aenc[8], Renc[8];
  fd_sgn_encode( Aenc, PA.X, PA.Y, zai );
  fd_sgn_encode( Renc, PR.X, PR.Y, zri );
  if( ok && !derive ) {
#pragma unroll
    for( int k=0; k<8; k++ ) Aenc[k] = fd_ld_u32_unaligned( blob + d.pub_off + 4*k );
  }

  uint64_t S[4];
  fd_sgn_finish( S, Renc, Aenc, M, sz, a, r );

  if( live ) {
    uint4 * so = (uint4 *)sig_out + 4UL*i;
    uint4 z4 = make_uint4( 0u, 0u, 0u, 0u );
    so[0] = ok ? make_uint4( Renc[0], Renc[1], Renc[2], Renc[3] ) : z4;
    so[1] = ok ? make_uint4( Renc[4], Renc[5], Renc[6], Renc[7] ) : z4;
    so[2] = ok ? make_uint4( (uint32_t)S[0], (uint32_t)(S[0]>>32), (uint32_t)S[1], (uint32_t)(S[1]>>32) ) : z4;
    so[3] = ok ? make_uint4( (uint32_t)S[2], (uint32_t)(S[2]>>32), (uint32_t)S[3], (uint32_t)(S[3]>>32) ) : z4;
    if( pub_out ) {
      uint4 * po = (uint4 *)pub_out + 2UL*i;
      po[0] = ok ? make_uint4( Aenc[0], Aenc[1], Aenc[2], Aenc[3] ) : z4;
      po[1] = ok ? make_uint4( Aenc[4], Aenc[5], Aenc[6], Aenc[7] ) : z4;
    }
    status[i] = ok ? FD_ED25519_SUCCESS : FD_ED25519_ERR_ARG;
  }
}

template<int BATCH>
__global__ void __launch_bounds__(FD_SGN_WG)
fd_k_sign( uint64_t n, uint8_t const * __restrict__ blob, uint64_t blob_sz, fd_ed25519_gpu_sign_desc_t const * __restrict__ sdesc,
           uint8_t * __restrict__ sig_out, uint8_t * __restrict__ pub_out, int32_t * __restrict__ status ) {
  __shared__ __attribute__((aligned(16))) int32_t lt[FD_SGN_COMB_DWS];
  fd_sgn_stage_comb( lt );
  fd_sign_body<BATCH>( n, blob, blob_sz, sdesc, sig_out, pub_out, status, (fd_sgn_lds_i32 *)lt );
}

/* hash != 0: the public key of seed in[32 i ..): SHA-512, clamp, [a]B,
   encode.  hash == 0: the encoding of [s]B for the raw scalar in[32 i ..). */
template<int BATCH>
__global__ void __launch_bounds__(FD_SGN_WG)
fd_k_public( uint64_t n, uint8_t const * __restrict__ in, uint8_t * __restrict__ out, int hash ) {
  __shared__ __attribute__((aligned(16))) int32_t lt[FD_SGN_COMB_DWS];
  fd_sgn_stage_comb( lt );
  uint64_t const i = (uint64_t)blockIdx.x * FD_SGN_WG + threadIdx.x;
  bool const live = i < n;
  uint4 lo = make_uint4( 0u, 0u, 0u, 0u ), hi = lo;
  if( live ) { lo = ((uint4 const *)in)[2UL*i]; hi = ((uint4 const *)in)[2UL*i+1UL]; }
  uint32_t s[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
  if( hash ) {                                   /* uniform */
    uint64_t seed[4], prefix[4];
#pragma unroll
    for( int k=0; k<4; k++ ) seed[k] = fd_bswap64( ((uint64_t)s[2*k+1] << 32) | s[2*k] );
    fd_sgn_expand( s, prefix, seed );
  }
  fd_sgn_p3_t P;
  fd_sgn_base_mul( P, s, (fd_sgn_lds_i32 *)lt );
  fd_gpu_fe_t z = P.Z, zi;
  if( !live ) fd_fe_set( z, 1 );
  fd_sgn_invert<BATCH>( zi, z );
  uint32_t enc[8];
  fd_sgn_encode( enc, P.X, P.Y, zi );
  if( live ) {
    ((uint4 *)out)[2UL*i]     = make_uint4( enc[0], enc[1], enc[2], enc[3] );
    ((uint4 *)out)[2UL*i+1UL] = make_uint4( enc[4], enc[5], enc[6], enc[7] );
  }
}

__global__ void __launch_bounds__(256)
fd_k_debug_muladd( uint64_t n, uint64_t const * __restrict__ k, uint64_t const * __restrict__ a, uint64_t const * __restrict__ r,
                   uint64_t * __restrict__ out ) {
  uint64_t const i = (uint64_t)blockIdx.x * 256UL + threadIdx.x;
  if( i >= n ) return;
  uint64_t kw[4], aw[4], rw[4], s[4];
#pragma unroll
  for( int j=0; j<4; j++ ) { kw[j] = k[4UL*i+j]; aw[j] = a[4UL*i+j]; rw[j] = r[4UL*i+j]; }
  fd_sgn_sc_muladd( s, kw, aw, rw );
#pragma unroll
  for( int j=0; j<4; j++ ) out[4UL*i+j] = s[j];
}

extern "C" hipError_t fd_ed25519_gpu_launch_sign( uint64_t n, uint8_t const * blob, uint64_t blob_sz, fd_ed25519_gpu_sign_desc_t const * sdesc,
                                                  uint8_t * sig_out, uint8_t * pub_out, int32_t * status, int batch_inv, hipStream_t stream ) {
  if( !n ) return hipSuccess;
  dim3 grid( (unsigned)((n + FD_SGN_WG - 1) / FD_SGN_WG) ), block( FD_SGN_WG );
  if( batch_inv ) hipLaunchKernelGGL( fd_k_sign<1>, grid, block, 0, stream, n, blob, blob_sz, sdesc, sig_out, pub_out, status );
  else            hipLaunchKernelGGL( fd_k_sign<0>, grid, block, 0, stream, n, blob, blob_sz, sdesc, sig_out, pub_out, status );
  return hipGetLastError();
}

extern "C" hipError_t fd_ed25519_gpu_launch_public( uint64_t n, uint8_t const * in, uint8_t * out, int hash, int batch_inv, hipStream_t stream ) {
  if( !n ) return hipSuccess;
  dim3 grid( (unsigned)((n + FD_SGN_WG - 1) / FD_SGN_WG) ), block( FD_SGN_WG );
  if( batch_inv ) hipLaunchKernelGGL( fd_k_public<1>, grid, block, 0, stream, n, in, out, hash );
  else            hipLaunchKernelGGL( fd_k_public<0>, grid, block, 0, stream, n, in, out, hash );
  return hipGetLastError();
}

extern "C" hipError_t fd_ed25519_gpu_launch_debug_muladd( uint64_t n, uint8_t const * k, uint8_t const * a, uint8_t const * r, uint8_t * out,
                                                          hipStream_t stream ) {
  if( !n ) return hipSuccess;
  hipLaunchKernelGGL( fd_k_debug_muladd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n,
                      (uint64_t const *)k, (uint64_t const *)a, (uint64_t const *)r, (uint64_t *)out );
  return hipGetLastError();
}
