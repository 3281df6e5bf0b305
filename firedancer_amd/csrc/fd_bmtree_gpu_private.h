#ifndef HEADER_fd_bmtree_gpu_private_h
#define HEADER_fd_bmtree_gpu_private_h

/* fd_bmtree_gpu_private.h -- between fd_bmtree_gpu.cpp (host side), the
   kernel unit fd_bmtree_gpu_kernels.hip and fd_poh_gpu.cpp (entries from
   leaves). */

#include <string.h>
#include <hip/hip_runtime.h>
#include "fd_bmtree_gpu.h"
#include "fd_poh_gpu.h"

/* fd_poh_gpu.cpp only: a tree without leaves is no tree (code 0, its root
   slot is not written) */
#define FD_BMTREE_GPU_SKIP_EMPTY (0x80000000U)

/* trees per block in the set-up kernels */
#define FD_BMTREE_TB 256U

/* One call's schedule.  Layer 0 is the leaf nodes, dense over all trees in
   the caller's order (tree t at first[t]); a tree with c > 1 nodes in layer
   l has ceil( c / 2 ) in layer l+1 and a tree with one node has none: it
   has written its root.  off + (l-1) (T+1) is the exclusive prefix of the
   per-tree node counts of layer l = 1..L, its entry T the layer's total.
   Nodes are eight host-order words; the layers alternate between node_a
   (layer 0, 2, ..) and node_b. */
typedef struct {
  uint32_t width, flags;
  uint32_t T, N;               /* trees, leaves */
  uint32_t L;                  /* merge launches: ceil( log2( min( leaf_max, N ) ) ) */
  uint32_t leaf_max, blob_sz;
  uint32_t NB;                 /* ceil( T / FD_BMTREE_TB ) */
  uint32_t const *             first;
  fd_bmtree_gpu_leaf_t const * leaves;
  uint8_t const *              blob;
  uint8_t *  roots;
  uint64_t   root_stride;
  int32_t *  codes;
  uint32_t * bad;              /* T words: after set-up, nonzero where the tree is refused or skipped */
  uint32_t * off;              /* L rows of T+1 */
  uint32_t * part;             /* L rows of NB: the blocks' sums, then their exclusive prefix */
  uint32_t * node_a;  uint32_t cap_a;   /* capacities in nodes */
  uint32_t * node_b;  uint32_t cap_b;
  uint8_t *  proofs;           /* the emit calls: leaf i's proof row at proofs + i proof_stride; else NULL */
  uint64_t   proof_stride;
} fd_bmtree_plan_t;

/* One from-proofs call: one lane per descriptor, no work memory. */
typedef struct {
  uint32_t width, flags;
  uint32_t n, blob_sz, depth_max;
  fd_bmtree_gpu_proof_t const * desc;
  uint8_t const *               blob;
  uint8_t *  roots;
  uint64_t   root_stride;
  int32_t *  codes;
} fd_bmtree_walk_plan_t;

static inline uint32_t fd_bmtree_ceil_log2( unsigned long n ) {
  uint32_t l = 0U;
  while( ( 1UL << l ) < n ) l++;
  return l;
}

/* fd_bmtree_gpu_work_sz's layout: fills the work pointers of p (T, N set)
   from base and returns the bytes used; rows = ceil_log2( N ) */
static inline unsigned long fd_bmtree_plan_layout( fd_bmtree_plan_t * p, uint8_t * base ) {
  unsigned long T = p->T, N = p->N, rows = fd_bmtree_ceil_log2( N ), NB = ( T + FD_BMTREE_TB - 1UL ) / FD_BMTREE_TB;
  unsigned long at = 0UL;
#define FD_BMTREE_TAKE(ptr,type,bytes) do { (ptr) = (type)( base + at ); at += ( (unsigned long)(bytes) + 15UL ) & ~15UL; } while(0)
  p->NB = (uint32_t)NB;
  p->cap_a = (uint32_t)N; p->cap_b = (uint32_t)( 2UL*N/3UL + 1UL );
  FD_BMTREE_TAKE( p->bad,    uint32_t *, 4UL*( T ? T : 1UL ) );
  FD_BMTREE_TAKE( p->off,    uint32_t *, 4UL*rows*( T + 1UL ) );
  FD_BMTREE_TAKE( p->part,   uint32_t *, 4UL*rows*( NB ? NB : 1UL ) );
  FD_BMTREE_TAKE( p->node_a, uint32_t *, 32UL*( N ? N : 1UL ) );
  FD_BMTREE_TAKE( p->node_b, uint32_t *, 32UL*(unsigned long)p->cap_b );
#undef FD_BMTREE_TAKE
  return at;
}

/* an upper bound of layer l's node count (l >= 1) from the shapes alone:
   the trees with more than 2^(l-1) leaves, each at most one node above its
   share */
static inline unsigned long fd_bmtree_layer_bound( unsigned long T, unsigned long N, uint32_t l ) {
  unsigned long act = N / ( ( 1UL << (l-1U) ) + 1UL );
  return ( N >> l ) + ( act < T ? act : T );
}

/* the plan of a call and its merge lanes: lanes[l] bounds layer l+1.  Here,
   and not in fd_bmtree_gpu.cpp, so that tests/bmtree_plan_harness.cpp runs
   the arithmetic the calls run. */
static inline void fd_bmtree_plan_make( fd_bmtree_plan_t * p, unsigned width, unsigned flags, unsigned long n_trees, unsigned long n_leaves,
                                        unsigned long blob_sz, unsigned long leaf_max, uint8_t * d_work, uint32_t lanes[32] ) {
  memset( p, 0, sizeof(*p) );
  p->width = width; p->flags = flags; p->T = (uint32_t)n_trees; p->N = (uint32_t)n_leaves;
  p->leaf_max = (uint32_t)( leaf_max < 0xffffffffUL ? leaf_max : 0xffffffffUL );
  p->blob_sz  = (uint32_t)blob_sz;
  p->L = fd_bmtree_ceil_log2( leaf_max < n_leaves ? leaf_max : n_leaves );
  fd_bmtree_plan_layout( p, d_work );
  for( uint32_t l=0U; l<p->L; l++ ) lanes[l] = (uint32_t)fd_bmtree_layer_bound( n_trees, n_leaves, l + 1U );
}

/* Queues the whole call on stream: clear, check, the three offset kernels,
   the leaf kernel, and merge launch l = 0..L-1 over lanes[l] lanes (an
   upper bound of layer l+1's node count; the lanes past the count leave).
   With p->proofs, gather launch l (one lane per leaf) goes before merge
   launch l: layer l is in its buffer only from merge launch l-1, which
   writes it, to merge launch l+1, which overwrites it. */
extern "C" hipError_t fd_bmtree_gpu_launch( fd_bmtree_plan_t const * p, uint32_t const * lanes, hipStream_t stream );

/* the one launch of a from-proofs call */
extern "C" hipError_t fd_bmtree_gpu_walk_launch( fd_bmtree_walk_plan_t const * p, hipStream_t stream );

/* fd_poh_gpu.cpp: entry i with leaves (first[i+1] > first[i]) whose tree is
   refused (tree_codes[i] != 0) or which lacks FD_POH_GPU_MIXIN gets a
   nonzero _pad in its device copy, so fd_k_poh refuses it unhashed */
extern "C" hipError_t fd_bmtree_gpu_poh_gate_launch( uint32_t n, uint32_t const * first, int32_t const * tree_codes,
                                                     fd_poh_gpu_entry_t * ent, hipStream_t stream );

/* the public device call with the private flags allowed */
extern "C" int fd_bmtree_gpu_roots_dev_flags( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                              uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                              void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                              unsigned long root_stride, int * d_codes, void * d_work, void * stream );

/* A packed tree batch as the device reads it: first[0..n] (the running sum
   of leaf_cnt) | leaves | blob, each part rounded up to 16 bytes.  Returns
   the parts' sizes and, unless h is NULL, writes the batch to h. */
typedef struct { unsigned long first_sz, leaf_sz, blob_sz; } fd_bmtree_staged_t;
extern "C" __attribute__((visibility("hidden")))
fd_bmtree_staged_t fd_bmtree_gpu_stage( uint8_t * h, unsigned long n, uint32_t const * leaf_cnt, unsigned long n_leaves,
                                        fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz );

#endif /* HEADER_fd_bmtree_gpu_private_h */
