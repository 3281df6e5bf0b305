/* fd_poh_gpu_kernels.hip -- fd_k_poh: Proof-of-History chains, one lane
   per entry (include/fd_poh_gpu.h).

   A translation unit of its own, outside the Makefile's KSRC: the verify
   kernels and their build id do not move with it.

   A chain is serial and its entries are independent, so a lane owns one
   entry from its first hash to its code and no lane talks to another: no
   LDS, no barrier, integer VALU only.  The hash bodies are fd_poh_core.h's
   (shared with the host routines): 64 rounds unrolled over a 16-word
   window in registers, the outer iteration loop kept a loop.  Between
   launches a lane's state and remaining count live in its HBM work row
   (fd_poh_gpu_private.h); a launch runs at most `chunk` hashes per lane, so
   no launch is unbounded, and the lane whose count runs out applies the
   mixin if flagged, compares with expect and writes the code. */

#include "fd_poh_core.h"
#include "fd_poh_gpu_private.h"

/* entry words (fd_poh_gpu_entry_t as 28 little-endian words) */
#define FD_POH_E_START   0
#define FD_POH_E_MIXIN   8
#define FD_POH_E_EXPECT 16
#define FD_POH_E_N      24
#define FD_POH_E_FLAGS  26
#define FD_POH_E_PAD    27

static_assert( sizeof(fd_poh_gpu_entry_t) == 112, "entry layout" );

extern "C" __global__ void __launch_bounds__(64)
fd_k_poh( uint32_t lanes, uint32_t first, uint32_t chunk, uint64_t n_max,
          fd_poh_gpu_entry_t const * __restrict__ ent, uint32_t const * __restrict__ order,
          uint32_t * __restrict__ work, int32_t * __restrict__ out, uint8_t * __restrict__ state_out ) {
  uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if( i >= lanes ) return;
  uint32_t * row = work + (uint64_t)i * FD_POH_ROW_WORDS;
  uint32_t   idx = order ? order[i] : i;
  uint2 const * e2 = (uint2 const *)( ent + idx );   /* entries are 8-byte aligned */

  uint32_t s[8];
  uint64_t rem;
  if( first ) {
    uint2 nn = e2[FD_POH_E_N/2], fp = e2[FD_POH_E_FLAGS/2];
    rem = ((uint64_t)nn.y << 32) | nn.x;
    if( ( fp.x & ~FD_POH_GPU_MIXIN ) | fp.y | (uint32_t)( rem > n_max ) ) {   /* refused: never hashed */
      out[idx] = FD_ED25519_ERR_ARG;
      if( state_out ) {
        uint4 * so = (uint4 *)( state_out + 32UL*(uint64_t)idx );
        so[0] = make_uint4( 0u, 0u, 0u, 0u ); so[1] = make_uint4( 0u, 0u, 0u, 0u );
      }
      *(uint4 *)( row + 8 ) = make_uint4( 0u, 0u, FD_POH_ROW_DONE, 0u );
      return;
    }
#pragma unroll
    for( int j=0; j<4; j++ ) {
      uint2 v = e2[FD_POH_E_START/2 + j];
      s[2*j] = __builtin_bswap32( v.x ); s[2*j+1] = __builtin_bswap32( v.y );
    }
  } else {
    uint4 t = *(uint4 const *)( row + 8 );
    if( t.z == FD_POH_ROW_DONE ) return;
    rem = ((uint64_t)t.y << 32) | t.x;
    uint4 lo = *(uint4 const *)( row ), hi = *(uint4 const *)( row + 4 );
    s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w; s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
  }

  uint32_t steps = rem < (uint64_t)chunk ? (uint32_t)rem : chunk;
  rem -= (uint64_t)steps;
#pragma clang loop unroll(disable)
  for( uint32_t k=0; k<steps; k++ ) fd_poh_step( s );

  if( rem ) {                                   /* more launches to come */
    *(uint4 *)( row     ) = make_uint4( s[0], s[1], s[2], s[3] );
    *(uint4 *)( row + 4 ) = make_uint4( s[4], s[5], s[6], s[7] );
    *(uint4 *)( row + 8 ) = make_uint4( (uint32_t)rem, (uint32_t)(rem >> 32), 0u, 0u );
    return;
  }

  if( e2[FD_POH_E_FLAGS/2].x & FD_POH_GPU_MIXIN ) {
    uint32_t m[8];
#pragma unroll
    for( int j=0; j<4; j++ ) {
      uint2 v = e2[FD_POH_E_MIXIN/2 + j];
      m[2*j] = __builtin_bswap32( v.x ); m[2*j+1] = __builtin_bswap32( v.y );
    }
    fd_poh_mix( s, m );
  }
  uint32_t diff = 0u;
#pragma unroll
  for( int j=0; j<4; j++ ) {
    uint2 v = e2[FD_POH_E_EXPECT/2 + j];
    diff |= ( __builtin_bswap32( v.x ) ^ s[2*j] ) | ( __builtin_bswap32( v.y ) ^ s[2*j+1] );
  }
  out[idx] = diff ? FD_POH_ERR_HASH : 0;
  if( state_out ) {
    uint4 * so = (uint4 *)( state_out + 32UL*(uint64_t)idx );
    so[0] = make_uint4( __builtin_bswap32( s[0] ), __builtin_bswap32( s[1] ), __builtin_bswap32( s[2] ), __builtin_bswap32( s[3] ) );
    so[1] = make_uint4( __builtin_bswap32( s[4] ), __builtin_bswap32( s[5] ), __builtin_bswap32( s[6] ), __builtin_bswap32( s[7] ) );
  }
  *(uint4 *)( row + 8 ) = make_uint4( 0u, 0u, FD_POH_ROW_DONE, 0u );
}

extern "C" hipError_t fd_poh_gpu_launch( uint32_t lanes, uint32_t first, uint32_t chunk, uint64_t n_max,
                                         fd_poh_gpu_entry_t const * ent, uint32_t const * order, uint32_t * work,
                                         int32_t * out, uint8_t * state_out, hipStream_t stream ) {
  if( !lanes ) return hipSuccess;
  hipLaunchKernelGGL( fd_k_poh, dim3((lanes + 63u) / 64u), dim3(64), 0, stream,
                      lanes, first, chunk, n_max, ent, order, work, out, state_out );
  return hipGetLastError();
}
