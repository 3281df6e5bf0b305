/* fd_bmtree_gpu_kernels.hip -- binary Merkle trees, many per call
   (include/fd_bmtree_gpu.h).

   A translation unit of its own, outside the Makefile's KSRC: the verify
   kernels and their build id do not move with it.

   The hash bodies are fd_bmtree_core.h's (shared with the host routines),
   on fd_poh_core.h's register-resident compression: integer VALU only, no
   LDS and no lane exchange in the hashing kernels.

   Schedule, compact per layer.  Layer 0 is the leaf nodes, one lane per
   leaf (fd_k_bmtree_leaf).  Every further layer keeps its nodes dense over
   all trees: a tree with c > 1 nodes has ceil( c / 2 ) in the next layer, a
   tree with one node has written its root and has none.  The exclusive
   prefixes of these counts, for every layer at once, are three small
   kernels (fd_k_bmtree_sums, _scan, _offsets: block sums, their scan, the
   offsets), so a merge launch (fd_k_bmtree_merge) runs one lane per OUTPUT
   node and all its lanes are busy whatever the tree sizes.  A lane finds
   its tree by a binary search in its layer's offsets.  Nothing is read back
   by the host: the launch count comes from the shapes.

   Refusals are decided before anything is hashed: fd_k_bmtree_check flags
   the trees of bad leaf descriptors (one lane per leaf), the set-up kernels
   add the count rules, and a refused tree has no node in any layer.

   Inclusion proofs.  The emit calls add fd_k_bmtree_proof_gather before
   each merge launch: the layers ping-pong between two buffers, so layer l
   is there only between merge launch l-1 and merge launch l+1, and the
   stream order is leaf, gather(0), merge(0), gather(1), merge(1), ...
   fd_k_bmtree_from_proof walks one proof per lane in one launch. */

#include "fd_bmtree_core.h"
#include "fd_bmtree_gpu_private.h"

static_assert( sizeof(fd_poh_gpu_entry_t) == 112, "entry layout" );
static_assert( FD_BMTREE_TB == 256U, "set-up block" );

/* the largest t in [0, T) with off[t] <= i (T >= 1) */
static __device__ __forceinline__ uint32_t fd_bmtree_find( uint32_t const * __restrict__ off, uint32_t T, uint32_t i ) {
  uint32_t lo = 0u, hi = T;
  while( hi - lo > 1u ) {
    uint32_t mid = lo + ( ( hi - lo ) >> 1 );
    if( off[mid] <= i ) lo = mid; else hi = mid;
  }
  return lo;
}

/* tree t's leaf count where its range is sane and within the count rules, else 0 */
static __device__ __forceinline__ uint32_t fd_bmtree_cnt_ok( fd_bmtree_plan_t const & p, uint32_t t ) {
  uint32_t f0 = p.first[t], f1 = p.first[t+1u];
  if( f1 < f0 || f1 > p.N ) return 0u;
  uint32_t c = f1 - f0;
  return c <= p.leaf_max ? c : 0u;
}

static __device__ __forceinline__ void fd_bmtree_root_store( fd_bmtree_plan_t const & p, uint32_t t, uint32_t const s[8] ) {
  uint32_t * r = (uint32_t *)( p.roots + (uint64_t)t * p.root_stride );
#pragma unroll
  for( int j=0; j<8; j++ ) r[j] = ( p.width == 32u || j < 5 ) ? __builtin_bswap32( s[j] ) : 0u;
}

/* one lane per leaf: a descriptor the header refuses flags its tree */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_check( fd_bmtree_plan_t p ) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if( i >= p.N ) return;
  fd_bmtree_gpu_leaf_t d = p.leaves[i];
  uint64_t end = (uint64_t)d.off + (uint64_t)d.sz;
  bool bad = end > (uint64_t)p.blob_sz || end > 0xffffffffUL || d.sz > FD_BMTREE_GPU_LEAF_SZ_MAX;
  if( p.flags & FD_BMTREE_GPU_LEAVES_ARE_NODES ) bad = bad || d.sz != p.width;
  if( bad ) p.bad[ fd_bmtree_find( p.first, p.T, i ) ] = 1u;
}

/* one lane per tree: the sums over each block of FD_BMTREE_TB trees of the
   node counts of layers 1..L */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_sums( fd_bmtree_plan_t p ) {
  __shared__ uint32_t acc[32];
  uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if( threadIdx.x < 32u ) acc[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t c = ( t < p.T && !p.bad[t] ) ? fd_bmtree_cnt_ok( p, t ) : 0u;
  for( uint32_t l=0u; l<p.L && c>1u; l++ ) {
    c = ( c + 1u ) >> 1;
    atomicAdd( &acc[l], c );
  }
  __syncthreads();
  if( threadIdx.x < p.L ) p.part[ (uint64_t)threadIdx.x * p.NB + blockIdx.x ] = acc[threadIdx.x];
}

/* block l: the exclusive prefix of row l of the block sums, in place, and
   the layer's total to off[l][T] */
extern "C" __global__ void __launch_bounds__(1024)
fd_k_bmtree_scan( fd_bmtree_plan_t p ) {
  __shared__ uint32_t sh[1024];
  uint32_t * row = p.part + (uint64_t)blockIdx.x * p.NB;
  uint32_t carry = 0u;
  for( uint32_t base=0u; base<p.NB; base+=1024u ) {
    uint32_t k = base + threadIdx.x;
    uint32_t v = k < p.NB ? row[k] : 0u;
    sh[threadIdx.x] = v;
    __syncthreads();
    for( uint32_t d=1u; d<1024u; d<<=1 ) {
      uint32_t u = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
      __syncthreads();
      sh[threadIdx.x] += u;
      __syncthreads();
    }
    if( k < p.NB ) row[k] = carry + sh[threadIdx.x] - v;
    carry += sh[1023];
    __syncthreads();
  }
  if( threadIdx.x == 0u ) p.off[ (uint64_t)blockIdx.x * ( p.T + 1u ) + p.T ] = carry;
}

/* one lane per tree: its offsets in layers 1..L, its code, and the zero
   root of a refused tree */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_offsets( fd_bmtree_plan_t p ) {
  __shared__ uint32_t sh[256];
  uint32_t t = blockIdx.x * 256u + threadIdx.x;
  uint32_t c = 0u;
  if( t < p.T ) {
    uint32_t raw = p.first[t+1u] - p.first[t];
    c = p.bad[t] ? 0u : fd_bmtree_cnt_ok( p, t );
    bool skip = ( p.flags & FD_BMTREE_GPU_SKIP_EMPTY ) && !raw;
    p.bad[t] = c ? 0u : 1u;
    p.codes[t] = ( c || skip ) ? 0 : FD_ED25519_ERR_ARG;
    if( !c && !skip ) {
      uint32_t z[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
      fd_bmtree_root_store( p, t, z );
    }
  }
  for( uint32_t l=0u; l<p.L; l++ ) {
    c = c > 1u ? ( c + 1u ) >> 1 : 0u;
    sh[threadIdx.x] = c;
    __syncthreads();
    for( uint32_t d=1u; d<256u; d<<=1 ) {
      uint32_t u = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
      __syncthreads();
      sh[threadIdx.x] += u;
      __syncthreads();
    }
    if( t < p.T ) p.off[ (uint64_t)l * ( p.T + 1u ) + t ] = p.part[ (uint64_t)l * p.NB + blockIdx.x ] + sh[threadIdx.x] - c;
    __syncthreads();
  }
}

/* one lane per leaf: its node to layer 0, and the root of a one-leaf tree.
   A wave whose leaves are all 64 bytes (signatures) takes the two-block
   body; otherwise the wave takes the general one. */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_leaf( fd_bmtree_plan_t p ) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if( i >= p.N ) return;
  uint32_t t = fd_bmtree_find( p.first, p.T, i );
  if( p.bad[t] ) return;
  fd_bmtree_gpu_leaf_t d = p.leaves[i];
  uint8_t const * src = p.blob + d.off;
  uint32_t s[8];
  if( p.flags & FD_BMTREE_GPU_LEAVES_ARE_NODES ) {
    s[5] = 0u; s[6] = 0u; s[7] = 0u;
    if( p.width == 32u ) fd_bmtree_load( s, src, 8 ); else fd_bmtree_load( s, src, 5 );
  } else if( __all( d.sz == 64u ) ) {
    uint32_t m[16];
    if( !( (uintptr_t)src & 3UL ) ) {
      uint32_t const * s4 = (uint32_t const *)src;
#pragma unroll
      for( int k=0; k<16; k++ ) m[k] = __builtin_bswap32( s4[k] );
    } else {
      fd_bmtree_load( m, src, 16 );
    }
    fd_bmtree_leaf64( s, m );
  } else {
    fd_bmtree_leaf( s, src, d.sz );
  }
  if( p.width == 20u ) { s[5] = 0u; s[6] = 0u; s[7] = 0u; }
  uint4 * dst = (uint4 *)( p.node_a + 8UL*(uint64_t)i );
  dst[0] = make_uint4( s[0], s[1], s[2], s[3] );
  dst[1] = make_uint4( s[4], s[5], s[6], s[7] );
  if( p.first[t+1u] - p.first[t] == 1u ) fd_bmtree_root_store( p, t, s );
}

/* merge launch l: layer l (src, offsets so; l = 0: the leaves, first) to
   layer l+1 (dst, offsets dn), one lane per node of layer l+1.  A tree
   whose layer l+1 has one node writes it as its root. */
template< uint32_t W > static __device__ __forceinline__ void
fd_bmtree_merge_body( fd_bmtree_plan_t const & p, uint32_t const * __restrict__ so, uint32_t const * __restrict__ dn,
                      uint32_t const * __restrict__ src, uint32_t src_cap, uint32_t * __restrict__ dst, uint32_t dst_cap ) {
  uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if( i >= dn[p.T] || i >= dst_cap ) return;
  uint32_t t  = fd_bmtree_find( dn, p.T, i );
  uint32_t j  = i - dn[t];
  uint32_t s0 = so[t], c = so[t+1u] - s0;         /* the tree's nodes in layer l */
  if( so[t+1u] > src_cap || 2u*j >= c ) return;   /* not with offsets as documented */
  uint32_t ia = s0 + 2u*j, ib = 2u*j + 1u < c ? ia + 1u : ia;
  uint4 const * pa = (uint4 const *)( src + 8UL*(uint64_t)ia );
  uint4 const * pb = (uint4 const *)( src + 8UL*(uint64_t)ib );
  uint4 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
  uint32_t a[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
  uint32_t b[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
  uint32_t s[8];
  if( W == 32u ) fd_bmtree_merge32( s, a, b );
  else         { fd_bmtree_merge20( s, a, b ); s[5] = 0u; s[6] = 0u; s[7] = 0u; }
  if( c <= 2u ) { fd_bmtree_root_store( p, t, s ); return; }
  uint4 * pd = (uint4 *)( dst + 8UL*(uint64_t)i );
  pd[0] = make_uint4( s[0], s[1], s[2], s[3] );
  pd[1] = make_uint4( s[4], s[5], s[6], s[7] );
}

extern "C" __global__ void __launch_bounds__(64)
fd_k_bmtree_merge32( fd_bmtree_plan_t p, uint32_t const * so, uint32_t const * dn, uint32_t const * src, uint32_t src_cap,
                     uint32_t * dst, uint32_t dst_cap ) {
  fd_bmtree_merge_body<32u>( p, so, dn, src, src_cap, dst, dst_cap );
}

extern "C" __global__ void __launch_bounds__(64)
fd_k_bmtree_merge20( fd_bmtree_plan_t p, uint32_t const * so, uint32_t const * dn, uint32_t const * src, uint32_t src_cap,
                     uint32_t * dst, uint32_t dst_cap ) {
  fd_bmtree_merge_body<20u>( p, so, dn, src, src_cap, dst, dst_cap );
}

/* gather launch l, before merge launch l: one lane per leaf writes node l
   of its proof, the sibling in layer l (src, offsets so; l = 0: the leaves,
   first) of the node on its path, or that node where it has no sibling, to
   its row at l W.  Dword stores only: rows and W are multiples of 4.  The
   lanes of refused trees and of trees of depth <= l leave. */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_proof_gather( fd_bmtree_plan_t p, uint32_t l, uint32_t const * so, uint32_t const * src, uint32_t src_cap ) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if( i >= p.N ) return;
  uint32_t t = fd_bmtree_find( p.first, p.T, i );
  if( p.bad[t] ) return;
  uint32_t f0 = p.first[t], f1 = p.first[t+1u];
  if( i < f0 || i >= f1 ) return;                 /* not with offsets as documented */
  uint32_t cl = fd_bmtree_layer_cnt( f1 - f0, l );
  if( cl <= 1u ) return;                          /* l >= D: the root is no proof node */
  uint32_t base = l ? so[t] : f0;
  uint64_t k = (uint64_t)base + fd_bmtree_proof_idx( ( i - f0 ) >> l, cl );
  if( k >= src_cap ) return;
  uint4 const * pn = (uint4 const *)( src + 8UL*k );
  uint4 n0 = pn[0], n1 = pn[1];
  uint32_t * row = (uint32_t *)( p.proofs + (uint64_t)i * p.proof_stride + (uint64_t)l * p.width );
  row[0] = __builtin_bswap32( n0.x ); row[1] = __builtin_bswap32( n0.y ); row[2] = __builtin_bswap32( n0.z );
  row[3] = __builtin_bswap32( n0.w ); row[4] = __builtin_bswap32( n1.x );
  if( p.width == 32u ) { row[5] = __builtin_bswap32( n1.y ); row[6] = __builtin_bswap32( n1.z ); row[7] = __builtin_bswap32( n1.w ); }
}

/* n big-endian words from 4 n bytes at any alignment, word loads where the
   address allows them */
static __device__ __forceinline__ void fd_bmtree_load_any( uint32_t * d, uint8_t const * q, int words ) {
  if( !( (uintptr_t)q & 3UL ) ) {
    uint32_t const * q4 = (uint32_t const *)q;
    for( int k=0; k<words; k++ ) d[k] = __builtin_bswap32( q4[k] );
  } else {
    fd_bmtree_load( d, q, words );
  }
}

/* One lane per proof: the descriptor's check (a refused lane writes its
   code and its zero root and leaves), the leaf node as in fd_k_bmtree_leaf,
   the walk to the lane's depth, the comparison, the root and the code.
   roots may lie inside blob (a part no descriptor reads), so neither is
   __restrict__. */
template< uint32_t W > static __device__ __forceinline__ void
fd_bmtree_walk_body( fd_bmtree_walk_plan_t const & p ) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if( i >= p.n ) return;
  fd_bmtree_gpu_proof_t d = p.desc[i];
  uint32_t * r = (uint32_t *)( p.roots + (uint64_t)i * p.root_stride );
  int nodes = !!( p.flags & FD_BMTREE_GPU_LEAVES_ARE_NODES );
  if( !fd_bmtree_proof_ok( W, nodes, p.blob_sz, p.depth_max, FD_BMTREE_GPU_LEAF_SZ_MAX, d.leaf_off, d.leaf_sz, d.proof_off, d.idx,
                           d.leaf_cnt, d.depth, d.expect_off, d.flags ) ) {
#pragma unroll
    for( int j=0; j<8; j++ ) r[j] = 0u;
    p.codes[i] = FD_ED25519_ERR_ARG;
    return;
  }
  constexpr int words = W == 32u ? 8 : 5;
  uint8_t const * src = p.blob + d.leaf_off;
  uint32_t s[8];
  if( nodes ) {
    fd_bmtree_load_any( s, src, words );
  } else if( __all( d.leaf_sz == 64u ) ) {
    uint32_t m[16];
    fd_bmtree_load_any( m, src, 16 );
    fd_bmtree_leaf64( s, m );
  } else {
    fd_bmtree_leaf( s, src, d.leaf_sz );
  }
  uint8_t const * q = p.blob + d.proof_off;
#pragma nounroll
  for( uint32_t l=0u; l<d.depth; l++, q+=W ) {
    int alone = d.leaf_cnt && fd_bmtree_no_sibling( d.idx >> l, fd_bmtree_layer_cnt( d.leaf_cnt, l ) );
    uint32_t pn[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    if( !alone ) fd_bmtree_load_any( pn, q, words );
    fd_bmtree_walk_step( W, s, pn, ( d.idx >> l ) & 1u, alone );
  }
  int32_t code = 0;
  if( d.flags & FD_BMTREE_GPU_PROOF_EXPECT ) {
    uint32_t e[8];
    fd_bmtree_load_any( e, p.blob + d.expect_off, words );
    uint32_t diff = 0u;
#pragma unroll
    for( int k=0; k<words; k++ ) diff |= e[k] ^ s[k];
    if( diff ) code = FD_BMTREE_ERR_PROOF;
  }
#pragma unroll
  for( int j=0; j<8; j++ ) r[j] = j < words ? __builtin_bswap32( s[j] ) : 0u;
  p.codes[i] = code;
}

extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_from_proof( fd_bmtree_walk_plan_t p ) {
  if( p.width == 32u ) fd_bmtree_walk_body<32u>( p ); else fd_bmtree_walk_body<20u>( p );
}

/* one lane per Proof-of-History entry (fd_bmtree_gpu_private.h) */
extern "C" __global__ void __launch_bounds__(256)
fd_k_bmtree_poh_gate( uint32_t n, uint32_t const * __restrict__ first, int32_t const * __restrict__ tree_codes,
                      fd_poh_gpu_entry_t * __restrict__ ent ) {
  uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if( i >= n ) return;
  if( first[i+1u] == first[i] ) return;
  if( tree_codes[i] || !( ent[i].flags & FD_POH_GPU_MIXIN ) ) ent[i]._pad = 1u;
}

extern "C" hipError_t fd_bmtree_gpu_launch( fd_bmtree_plan_t const * pp, uint32_t const * lanes, hipStream_t stream ) {
  fd_bmtree_plan_t p = *pp;
  if( !p.T ) return hipSuccess;
  hipError_t e = hipMemsetAsync( p.bad, 0, 4UL*p.T, stream );
  if( e != hipSuccess ) return e;
  if( p.N ) hipLaunchKernelGGL( fd_k_bmtree_check, dim3((p.N + 255u) / 256u), dim3(256), 0, stream, p );
  if( p.L ) {
    hipLaunchKernelGGL( fd_k_bmtree_sums, dim3(p.NB), dim3(256), 0, stream, p );
    hipLaunchKernelGGL( fd_k_bmtree_scan, dim3(p.L), dim3(1024), 0, stream, p );
  }
  hipLaunchKernelGGL( fd_k_bmtree_offsets, dim3(p.NB), dim3(256), 0, stream, p );
  if( p.N ) hipLaunchKernelGGL( fd_k_bmtree_leaf, dim3((p.N + 255u) / 256u), dim3(256), 0, stream, p );
  for( uint32_t l=0u; l<p.L; l++ ) {
    uint32_t const * so = l ? p.off + (uint64_t)(l-1u) * ( p.T + 1u ) : p.first;
    uint32_t const * dn = p.off + (uint64_t)l * ( p.T + 1u );
    uint32_t * src = ( l & 1u ) ? p.node_b : p.node_a;  uint32_t src_cap = ( l & 1u ) ? p.cap_b : p.cap_a;
    uint32_t * dst = ( l & 1u ) ? p.node_a : p.node_b;  uint32_t dst_cap = ( l & 1u ) ? p.cap_a : p.cap_b;
    uint32_t n = lanes[l] < dst_cap ? lanes[l] : dst_cap;
    if( !n ) continue;                            /* no tree has two nodes in layer l: nothing to gather either */
    if( p.proofs && p.N ) hipLaunchKernelGGL( fd_k_bmtree_proof_gather, dim3((p.N + 255u) / 256u), dim3(256), 0, stream, p, l, so, src, src_cap );
    if( p.width == 32u ) hipLaunchKernelGGL( fd_k_bmtree_merge32, dim3((n + 63u) / 64u), dim3(64), 0, stream, p, so, dn, src, src_cap, dst, dst_cap );
    else                 hipLaunchKernelGGL( fd_k_bmtree_merge20, dim3((n + 63u) / 64u), dim3(64), 0, stream, p, so, dn, src, src_cap, dst, dst_cap );
  }
  return hipGetLastError();
}

extern "C" hipError_t fd_bmtree_gpu_walk_launch( fd_bmtree_walk_plan_t const * pp, hipStream_t stream ) {
  if( !pp->n ) return hipSuccess;
  hipLaunchKernelGGL( fd_k_bmtree_from_proof, dim3((pp->n + 255u) / 256u), dim3(256), 0, stream, *pp );
  return hipGetLastError();
}

extern "C" hipError_t fd_bmtree_gpu_poh_gate_launch( uint32_t n, uint32_t const * first, int32_t const * tree_codes,
                                                     fd_poh_gpu_entry_t * ent, hipStream_t stream ) {
  if( !n ) return hipSuccess;
  hipLaunchKernelGGL( fd_k_bmtree_poh_gate, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, first, tree_codes, ent );
  return hipGetLastError();
}
