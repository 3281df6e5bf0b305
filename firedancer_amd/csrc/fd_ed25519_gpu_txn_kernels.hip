/* fd_ed25519_gpu_txn_kernels.hip -- whole transactions on the device
   (include/fd_ed25519_gpu_txn.h): parse, scan, expand, reduce around the
   unchanged verify pipeline.  A translation unit of its own, outside the
   Makefile's KSRC, so the verify kernels' build id does not move with it.

   All four kernels are bandwidth- and latency-light next to the verify
   pipeline they feed: the parser reads a few cache lines of each payload
   (the counts, one byte per instruction account), the others 8-24 bytes
   per transaction and 16 per signature.

   fd_k_txn_ring_front and fd_k_txn_ring_reduce are the ring's pair
   (fd_ed25519_gpu_submit_txns): one launch in front of the verify pipeline
   and one behind it, on a slot layout the host computed. */

#include "fd_ed25519_gpu_txn_private.h"
#include "fd_txn_core.h"

#define FD_TXN_SCAN_WG 1024

/* the tail-slot descriptor: fails fd_desc_in for every blob_sz < 2^32 */
#define FD_TXN_DESC_FILL make_uint4( 0xffffffffU, 0xffffffffU, 0U, 0U )

/* inclusive scan of v over the 64 lanes of a wave */
static __device__ __forceinline__ uint32_t fd_wave_scan( uint32_t v, uint32_t lane ) {
#pragma unroll
  for( int d=1; d<64; d<<=1 ) {
    uint32_t u = (uint32_t)__shfl_up( (int)v, d, 64 );
    if( lane >= (uint32_t)d ) v += u;
  }
  return v;
}

/* One lane per transaction: the parser core on blob[off, off+sz) (an entry
   outside blob[0, blob_sz) is never dereferenced), the result's parse
   fields, the optional descriptor, and the block's exclusive scan of the
   signature counts (every thread of the block takes part, also those past
   n_txn, with a count of 0). */
__global__ void __launch_bounds__( FD_TXN_WG )
fd_k_txn_parse( uint64_t n_txn, uint8_t const * __restrict__ blob, uint64_t blob_sz, fd_ed25519_gpu_txn_t const * __restrict__ txn,
                fd_ed25519_gpu_txn_result_t * __restrict__ res, uint8_t * __restrict__ txn_out, uint64_t txn_out_stride,
                fd_txn_meta_t * __restrict__ meta, uint32_t * __restrict__ part ) {
  __shared__ uint32_t wsum[ FD_TXN_WG / 64 ];
  uint64_t t = (uint64_t)blockIdx.x * FD_TXN_WG + threadIdx.x;
  uint32_t cnt = 0, acct_off = 0;
  if( t < n_txn ) {
    fd_ed25519_gpu_txn_t e = txn[ t ];
    fd_txn_core_sum_t sum;
    int32_t status;
    if( (uint64_t)e.off + (uint64_t)e.sz > blob_sz ) {
      sum.tag = 0; sum.footprint = 0; sum.reject_line = 0; sum.acct_addr_off = 0; sum.sig_cnt = 0; sum.version = FD_TXN_VLEGACY;
      status = FD_ED25519_ERR_ARG;
    } else {
      unsigned long fp = fd_txn_core_parse( blob + e.off, (unsigned long)e.sz, txn_out ? txn_out + t * txn_out_stride : (uint8_t *)0,
                                            (unsigned long)txn_out_stride, &sum );
      status = fp ? FD_ED25519_SUCCESS : FD_ED25519_ERR_TXN;
    }
    cnt = sum.sig_cnt; acct_off = sum.acct_addr_off;
    /* the 24-byte result as three 8-byte stores (d_res is 8-byte aligned) */
    uint32_t fp16 = sum.footprint > 0xffffU ? 0xffffU : sum.footprint;
    uint64_t * r = (uint64_t *)( res + t );
    r[0] = (uint64_t)(uint32_t)status;                    /* status | sig_base (set by fd_k_txn_expand) << 32 */
    r[1] = sum.tag;
    r[2] = (uint64_t)fp16 | ((uint64_t)sum.reject_line << 16) | ((uint64_t)sum.sig_cnt << 32) | ((uint64_t)sum.version << 40);
  }
  uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t inc = fd_wave_scan( cnt, lane );
  if( lane == 63u ) wsum[ w ] = inc;
  __syncthreads();
  uint32_t woff = 0;
  for( uint32_t k=0; k<w; k++ ) woff += wsum[ k ];
  if( t < n_txn ) meta[ t ] = make_uint2( cnt | (acct_off << 16), woff + inc - cnt );
  if( threadIdx.x == FD_TXN_WG - 1 ) part[ blockIdx.x ] = woff + inc;
}

/* Exclusive scan, in place, of the nblk block sums; part[nblk] = the
   total.  One block walks them FD_TXN_SCAN_WG at a time with a running
   carry, so any nblk works (2^20 transactions are 4,096 sums: four
   rounds). */
__global__ void __launch_bounds__( FD_TXN_SCAN_WG )
fd_k_txn_scan( uint64_t nblk, uint32_t * __restrict__ part ) {
  __shared__ uint32_t wsum[ FD_TXN_SCAN_WG / 64 ];
  uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for( uint64_t base=0; base<nblk; base+=FD_TXN_SCAN_WG ) {
    uint64_t i = base + threadIdx.x;
    uint32_t v = i < nblk ? part[ i ] : 0u;
    uint32_t inc = fd_wave_scan( v, lane );
    if( lane == 63u ) wsum[ w ] = inc;
    __syncthreads();
    uint32_t woff = 0, all = 0;
    for( uint32_t k=0; k<FD_TXN_SCAN_WG/64; k++ ) { if( k < w ) woff += wsum[ k ]; all += wsum[ k ]; }
    if( i < nblk ) part[ i ] = carry + woff + inc - v;
    carry += all;
    __syncthreads();      /* wsum is rewritten by the next round */
  }
  if( threadIdx.x == 0 ) part[ nblk ] = carry;
}

/* Thread i does two jobs.  As transaction i: its sig_base, and if its
   signatures fit below sig_cap its descriptors (any count up to 127: a
   plain loop), else ERR_ARG; the first transaction that does not fit also
   fills the slots from its base to sig_cap.  As slot i: a tail slot past
   the total is filled.  part[nblk+1] = the number of slots transactions
   took. */
__global__ void __launch_bounds__( 256 )
fd_k_txn_expand( uint64_t n_txn, fd_ed25519_gpu_txn_t const * __restrict__ txn, uint64_t sig_cap,
                 fd_ed25519_gpu_txn_result_t * __restrict__ res, fd_txn_meta_t const * __restrict__ meta,
                 uint32_t * __restrict__ part, uint4 * __restrict__ desc ) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint64_t nblk = ( n_txn + FD_TXN_WG - 1UL ) / FD_TXN_WG;
  uint64_t total = part[ nblk ];
  if( i == 0 && total <= sig_cap ) part[ nblk + 1UL ] = (uint32_t)total;
  if( i >= total && i < sig_cap ) desc[ i ] = FD_TXN_DESC_FILL;
  if( i >= n_txn ) return;
  fd_txn_meta_t m = meta[ i ];
  uint64_t cnt = m.x & 0xffu, base = (uint64_t)part[ i / FD_TXN_WG ] + m.y;
  res[ i ].sig_base = (uint32_t)base;
  if( !cnt ) return;
  if( base + cnt > sig_cap ) {
    res[ i ].status = FD_ED25519_ERR_ARG;
    if( base <= sig_cap ) {            /* the first that does not fit: every later one starts past sig_cap */
      part[ nblk + 1UL ] = (uint32_t)base;
      for( uint64_t s=base; s<sig_cap; s++ ) desc[ s ] = FD_TXN_DESC_FILL;
    }
    return;
  }
  fd_ed25519_gpu_txn_t e = txn[ i ];
  uint32_t acct = e.off + ( m.x >> 16 );
  uint32_t msg  = 1u + 64u * (uint32_t)cnt;       /* signature_off is 1, message_off follows the signatures */
  for( uint64_t k=0; k<cnt; k++ )
    desc[ base + k ] = make_uint4( e.off + 1u + 64u * (uint32_t)k, acct + 32u * (uint32_t)k, e.off + msg, e.sz - msg );
}

/* The first nonzero code of a transaction's slots, in signature order.
   Only transactions that got slots (parsed, status still SUCCESS) are
   touched; tail slots belong to nobody. */
__global__ void __launch_bounds__( 256 )
fd_k_txn_reduce( uint64_t n_txn, fd_ed25519_gpu_txn_result_t * __restrict__ res, int32_t const * __restrict__ codes ) {
  uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if( t >= n_txn ) return;
  uint32_t cnt = res[ t ].sig_cnt;
  if( !cnt || res[ t ].status != FD_ED25519_SUCCESS ) return;
  int32_t const * c = codes + res[ t ].sig_base;
  for( uint32_t k=0; k<cnt; k++ ) {
    int32_t v = c[ k ];
    if( v ) { res[ t ].status = v; return; }
  }
}

/* The ring's front end (fd_ed25519_gpu_submit_txns): parse and expand in
   one launch, for batches whose slot layout the host computed
   (fd_ed25519_gpu_txn_claims): bases[t] is transaction t's first slot,
   bases[t+1] - bases[t] the slots it claims (its first payload byte),
   bases[n_txn] = n_sig.  No workgroup reads anything another one writes.

   Lane i of block b parses transaction 256 b + i, writes its result with
   sig_base = bases[t], and leaves in LDS what its slots need.  After the
   barrier the block's lanes walk the block's slots [bases[256 b],
   bases[min(256 (b+1), n_txn)]), one lane per slot, 256 a round: the owner
   is the last transaction of the block whose base is <= the slot (a
   binary search over the bases in LDS), so a wave stores 64 consecutive
   descriptors as one 1 KiB run whatever the counts are.  A transaction
   that claims slots but does not parse (or, if the bytes changed under the
   host, parses to another count than it claimed: FD_ED25519_ERR_ARG) gets
   the fill descriptor in each.  Slots are clamped to [0, n_sig), so bases
   that are not what the host routine writes cannot send a store outside
   desc[0, n_sig). */
#define FD_TXN_RING_PARSED 0x80000000U
__global__ void __launch_bounds__( FD_TXN_WG )
fd_k_txn_ring_front( uint32_t n_txn, uint32_t n_sig, uint8_t const * __restrict__ blob, uint64_t blob_sz,
                     fd_ed25519_gpu_txn_t const * __restrict__ txn, uint32_t const * __restrict__ bases,
                     fd_ed25519_gpu_txn_result_t * __restrict__ res, uint4 * __restrict__ desc ) {
  __shared__ uint32_t s_base[ FD_TXN_WG + 1 ];
  __shared__ uint32_t s_off [ FD_TXN_WG ];
  __shared__ uint32_t s_sz  [ FD_TXN_WG ];
  __shared__ uint32_t s_acct[ FD_TXN_WG ];   /* acct_addr_off | FD_TXN_RING_PARSED, or 0: fill */
  uint32_t t0 = blockIdx.x * (uint32_t)FD_TXN_WG;
  uint32_t nb = n_txn - t0 < (uint32_t)FD_TXN_WG ? n_txn - t0 : (uint32_t)FD_TXN_WG;   /* the grid covers n_txn: t0 < n_txn */
  uint32_t i  = threadIdx.x;
  if( i < nb ) {
    uint32_t t = t0 + i;
    fd_ed25519_gpu_txn_t e = txn[ t ];
    uint32_t base = bases[ t ], claim = bases[ t + 1U ] - base;
    fd_txn_core_sum_t sum;
    int32_t status;
    if( (uint64_t)e.off + (uint64_t)e.sz > blob_sz ) {
      sum.tag = 0; sum.footprint = 0; sum.reject_line = 0; sum.acct_addr_off = 0; sum.sig_cnt = 0; sum.version = FD_TXN_VLEGACY;
      status = FD_ED25519_ERR_ARG;
    } else {
      unsigned long fp = fd_txn_core_parse( blob + e.off, (unsigned long)e.sz, (void *)0, 0UL, &sum );
      status = fp ? FD_ED25519_SUCCESS : FD_ED25519_ERR_TXN;
      if( fp && (uint32_t)sum.sig_cnt != claim ) {   /* not the bytes the host laid the slots out from */
        sum.tag = 0; sum.footprint = 0; sum.reject_line = 0; sum.acct_addr_off = 0; sum.sig_cnt = 0; sum.version = FD_TXN_VLEGACY;
        status = FD_ED25519_ERR_ARG;
      }
    }
    uint32_t fp16 = sum.footprint > 0xffffU ? 0xffffU : sum.footprint;
    uint64_t * r = (uint64_t *)( res + t );
    r[0] = (uint64_t)(uint32_t)status | ((uint64_t)base << 32);
    r[1] = sum.tag;
    r[2] = (uint64_t)fp16 | ((uint64_t)sum.reject_line << 16) | ((uint64_t)sum.sig_cnt << 32) | ((uint64_t)sum.version << 40);
    s_base[ i ] = base;
    s_off [ i ] = e.off;
    s_sz  [ i ] = e.sz;
    s_acct[ i ] = status == FD_ED25519_SUCCESS ? ( (uint32_t)sum.acct_addr_off | FD_TXN_RING_PARSED ) : 0U;
    if( i == nb - 1U ) s_base[ nb ] = base + claim;
  }
  __syncthreads();
  uint32_t lo = s_base[ 0 ], hi = s_base[ nb ];
  if( hi > n_sig ) hi = n_sig;
  for( uint32_t s=lo+i; s<hi; s+=(uint32_t)FD_TXN_WG ) {
    /* the last j in [0, nb) with s_base[j] <= s (s_base[0] = lo <= s) */
    uint32_t a = 0U, b = nb;
    while( b - a > 1U ) {
      uint32_t m = ( a + b ) >> 1;
      if( s_base[ m ] <= s ) a = m; else b = m;
    }
    uint32_t k = s - s_base[ a ], cnt = s_base[ a + 1U ] - s_base[ a ], acct = s_acct[ a ];
    uint4 d = FD_TXN_DESC_FILL;
    if( ( acct & FD_TXN_RING_PARSED ) && k < cnt ) {
      uint32_t off = s_off[ a ], msg = 1U + 64U * cnt;
      d = make_uint4( off + 1U + 64U * k, off + ( acct & 0xffffU ) + 32U * k, off + msg, s_sz[ a ] - msg );
    }
    desc[ s ] = d;
  }
}

/* fd_k_txn_reduce for the ring: the final result of every transaction goes
   to `out` (the slot's mapped pinned results), so the host reads them with
   no copy behind the kernel.  `codes` may be the slot's pinned h_out: the
   codes are fetched eight at a time, so a transaction of up to eight
   signatures costs one round trip over the link, not one per signature. */
__global__ void __launch_bounds__( 256 )
fd_k_txn_ring_reduce( uint32_t n_txn, uint32_t n_sig, fd_ed25519_gpu_txn_result_t const * __restrict__ res,
                      int32_t const * __restrict__ codes, fd_ed25519_gpu_txn_result_t * __restrict__ out ) {
  uint32_t t = blockIdx.x * 256U + threadIdx.x;
  if( t >= n_txn ) return;
  uint64_t const * r = (uint64_t const *)( res + t );
  uint64_t r0 = r[0], r1 = r[1], r2 = r[2];
  uint32_t cnt = (uint32_t)( r2 >> 32 ) & 0xffU, base = (uint32_t)( r0 >> 32 );
  int32_t status = (int32_t)(uint32_t)r0;
  if( cnt && status == FD_ED25519_SUCCESS && base <= n_sig && cnt <= n_sig - base ) {
    int32_t const * c = codes + base;
    for( uint32_t k0=0U; k0<cnt && !status; k0+=8U ) {
      int32_t v[8];
#pragma unroll
      for( uint32_t j=0U; j<8U; j++ ) v[j] = k0 + j < cnt ? c[ k0 + j ] : 0;
#pragma unroll
      for( uint32_t j=0U; j<8U; j++ ) if( !status && v[j] ) status = v[j];
    }
  }
  uint64_t * o = (uint64_t *)( out + t );
  o[0] = ( r0 & 0xffffffff00000000UL ) | (uint64_t)(uint32_t)status;
  o[1] = r1;
  o[2] = r2;
}

extern "C" hipError_t
fd_ed25519_gpu_launch_txn_ring_front( uint64_t n_txn, uint64_t n_sig, uint8_t const * blob, uint64_t blob_sz,
                                      fd_ed25519_gpu_txn_t const * txn, uint32_t const * bases, fd_ed25519_gpu_txn_result_t * res,
                                      fd_ed25519_gpu_desc_t * desc, hipStream_t stream ) {
  if( !n_txn || n_txn > FD_TXN_MAX || n_sig > 0xffffffffUL ) return hipErrorInvalidValue;
  hipLaunchKernelGGL( fd_k_txn_ring_front, dim3((unsigned)((n_txn + FD_TXN_WG - 1UL) / FD_TXN_WG)), dim3((unsigned)FD_TXN_WG), 0, stream,
                      (uint32_t)n_txn, (uint32_t)n_sig, blob, blob_sz, txn, bases, res, (uint4 *)desc );
  return hipGetLastError();
}

extern "C" hipError_t
fd_ed25519_gpu_launch_txn_ring_reduce( uint64_t n_txn, uint64_t n_sig, fd_ed25519_gpu_txn_result_t const * res, int32_t const * codes,
                                       fd_ed25519_gpu_txn_result_t * out, hipStream_t stream ) {
  if( !n_txn || n_txn > FD_TXN_MAX || n_sig > 0xffffffffUL ) return hipErrorInvalidValue;
  hipLaunchKernelGGL( fd_k_txn_ring_reduce, dim3((unsigned)((n_txn + 255UL) / 256UL)), dim3(256), 0, stream,
                      (uint32_t)n_txn, (uint32_t)n_sig, res, codes, out );
  return hipGetLastError();
}

extern "C" hipError_t
fd_ed25519_gpu_launch_txn_front( uint64_t n_txn, uint8_t const * blob, uint64_t blob_sz, fd_ed25519_gpu_txn_t const * txn,
                                 uint64_t sig_cap, fd_ed25519_gpu_txn_result_t * res, uint8_t * txn_out, uint64_t txn_out_stride,
                                 fd_txn_meta_t * meta, uint32_t * part, fd_ed25519_gpu_desc_t * desc, hipStream_t stream,
                                 hipEvent_t const * ev ) {
  hipError_t e;
  uint64_t nblk = ( n_txn + FD_TXN_WG - 1UL ) / FD_TXN_WG;
  uint64_t nexp = n_txn > sig_cap ? n_txn : sig_cap;
  if( ev && (e = hipEventRecord( ev[0], stream )) != hipSuccess ) return e;
  hipLaunchKernelGGL( fd_k_txn_parse, dim3((unsigned)nblk), dim3((unsigned)FD_TXN_WG), 0, stream, n_txn, blob, blob_sz, txn, res, txn_out,
                      txn_out_stride, meta, part );
  if( ev && (e = hipEventRecord( ev[1], stream )) != hipSuccess ) return e;
  hipLaunchKernelGGL( fd_k_txn_scan, dim3(1), dim3(FD_TXN_SCAN_WG), 0, stream, nblk, part );
  if( ev && (e = hipEventRecord( ev[2], stream )) != hipSuccess ) return e;
  hipLaunchKernelGGL( fd_k_txn_expand, dim3((unsigned)((nexp + 255UL) / 256UL)), dim3(256), 0, stream, n_txn, txn, sig_cap, res, meta, part,
                      (uint4 *)desc );
  if( ev && (e = hipEventRecord( ev[3], stream )) != hipSuccess ) return e;
  return hipGetLastError();
}

extern "C" hipError_t
fd_ed25519_gpu_launch_txn_reduce( uint64_t n_txn, fd_ed25519_gpu_txn_result_t * res, int32_t const * codes, hipStream_t stream ) {
  hipLaunchKernelGGL( fd_k_txn_reduce, dim3((unsigned)((n_txn + 255UL) / 256UL)), dim3(256), 0, stream, n_txn, res, codes );
  return hipGetLastError();
}
