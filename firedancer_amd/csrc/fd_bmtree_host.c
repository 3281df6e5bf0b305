/* fd_bmtree_host.c -- binary Merkle trees on the host
   (include/fd_bmtree_gpu.h): the reference's node and commit interface
   (src/ballet/bmtree/fd_bmtree_tmpl.c) at both widths, built from the
   SHA-256 bodies the device kernels use (fd_bmtree_core.h), and the batch
   semantics on host threads (fd_bmtree_roots_batch, and for inclusion
   proofs fd_bmtree_proofs_batch and fd_bmtree_from_proofs_batch: the
   bench's yardsticks and the CPU tests' subjects).  No device code. */

#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include "fd_bmtree_gpu.h"
#include "fd_bmtree_core.h"

#define EXPORT __attribute__((visibility("default")))

_Static_assert( sizeof(fd_bmtree20_commit_t) == FD_BMTREE20_COMMIT_FOOTPRINT && _Alignof(fd_bmtree20_commit_t) == FD_BMTREE20_COMMIT_ALIGN, "commit20" );
_Static_assert( sizeof(fd_bmtree32_commit_t) == FD_BMTREE32_COMMIT_FOOTPRINT && _Alignof(fd_bmtree32_commit_t) == FD_BMTREE32_COMMIT_ALIGN, "commit32" );
_Static_assert( sizeof(fd_bmtree_gpu_leaf_t) == 8, "leaf descriptor" );
_Static_assert( sizeof(fd_bmtree_gpu_proof_t) == 32, "proof descriptor" );

/* Both widths share one body over this view: the two commit structs have
   one layout, and this file reads and writes a commitment through the
   view only. */
typedef struct { uint8_t hash[32]; } fd_bmtree_hnode_t;
typedef struct { unsigned long leaf_cnt; unsigned long _pad[3]; fd_bmtree_hnode_t node_buf[63]; } fd_bmtree_hcommit_t;
_Static_assert( sizeof(fd_bmtree_hcommit_t) == 2048, "commit view" );

static void fd_bmtree_hleaf( uint8_t * out32, void const * data, unsigned long sz ) {
  uint32_t s[8];
  fd_bmtree_leaf( s, (uint8_t const *)data, (uint32_t)sz );
  fd_poh_store( out32, s );
}

/* out <- branch( a, b ) at width W, out may be a or b; all 32 bytes of out
   are written, [W,32) with digest bytes the tree never reads */
static void fd_bmtree_hmerge( unsigned W, uint8_t * out, uint8_t const * a, uint8_t const * b ) {
  uint32_t s[8], x[8], y[8];
  if( W == 32U ) {
    fd_bmtree_load( x, a, 8 ); fd_bmtree_load( y, b, 8 );
    fd_bmtree_merge32( s, x, y );
  } else {
    fd_bmtree_load( x, a, 5 ); fd_bmtree_load( y, b, 5 );
    fd_bmtree_merge20( s, x, y );
  }
  fd_poh_store( out, s );
}

/* One more leaf: it climbs for as long as it completes a pair, merging
   with the left sibling parked at each layer, and parks where it is a left
   child itself. */
static void fd_bmtree_hpush( unsigned W, fd_bmtree_hcommit_t * c, uint8_t const * leaf ) {
  uint8_t cur[32];
  memcpy( cur, leaf, 32 );
  unsigned long pos = c->leaf_cnt++;              /* the leaf's index; bit l: a right child at layer l */
  unsigned layer = 0U;
  for( ; pos & 1UL; pos >>= 1, layer++ ) fd_bmtree_hmerge( W, cur, c->node_buf[layer].hash, cur );
  memcpy( c->node_buf[layer].hash, cur, 32 );
}

/* The root of the leaves so far, left in node_buf at the root's layer.
   The parked nodes are visited bottom up; the running node is merged with
   itself where its layer has no node parked to its left. */
static uint8_t * fd_bmtree_hfini( unsigned W, fd_bmtree_hcommit_t * c ) {
  unsigned long n = c->leaf_cnt;
  unsigned layer = 0U;
  while( !( ( n >> layer ) & 1UL ) ) layer++;     /* the lowest parked node (n >= 1) */
  unsigned long cnt = n >> layer;                 /* nodes of this layer, the running one last: odd */
  if( cnt == 1UL ) return c->node_buf[layer].hash;      /* a power of two: the parked node is the root */
  uint8_t cur[32];
  memcpy( cur, c->node_buf[layer].hash, 32 );
  while( cnt > 1UL ) {
    if( cnt & 1UL ) fd_bmtree_hmerge( W, cur, cur, cur );
    else            fd_bmtree_hmerge( W, cur, c->node_buf[layer].hash, cur );
    layer++; cnt = ( cnt + 1UL ) >> 1;
  }
  memcpy( c->node_buf[layer].hash, cur, 32 );
  return c->node_buf[layer].hash;
}

#define FD_BMTREE_HOST_API( W )                                                                                          \
EXPORT fd_bmtree##W##_node_t * fd_bmtree##W##_hash_leaf( fd_bmtree##W##_node_t * node, void const * data, unsigned long data_sz ) { \
  fd_bmtree_hleaf( node->hash, data, data_sz );                                                                          \
  return node;                                                                                                           \
}                                                                                                                        \
EXPORT unsigned long fd_bmtree##W##_commit_align    ( void ) { return FD_BMTREE##W##_COMMIT_ALIGN; }                      \
EXPORT unsigned long fd_bmtree##W##_commit_footprint( void ) { return FD_BMTREE##W##_COMMIT_FOOTPRINT; }                  \
EXPORT fd_bmtree##W##_commit_t * fd_bmtree##W##_commit_init( void * mem ) {                                              \
  ((fd_bmtree_hcommit_t *)mem)->leaf_cnt = 0UL;                                                                          \
  return (fd_bmtree##W##_commit_t *)mem;                                                                                 \
}                                                                                                                        \
EXPORT unsigned long fd_bmtree##W##_commit_leaf_cnt( fd_bmtree##W##_commit_t const * bmt ) {                             \
  return ((fd_bmtree_hcommit_t const *)bmt)->leaf_cnt;                                                                   \
}                                                                                                                        \
EXPORT fd_bmtree##W##_commit_t * fd_bmtree##W##_commit_append( fd_bmtree##W##_commit_t * bmt,                            \
                                                               fd_bmtree##W##_node_t const * leaf, unsigned long leaf_cnt ) { \
  for( unsigned long i=0UL; i<leaf_cnt; i++ ) fd_bmtree_hpush( W##U, (fd_bmtree_hcommit_t *)bmt, leaf[i].hash );         \
  return bmt;                                                                                                            \
}                                                                                                                        \
EXPORT uint8_t * fd_bmtree##W##_commit_fini( fd_bmtree##W##_commit_t * bmt ) {                                           \
  return fd_bmtree_hfini( W##U, (fd_bmtree_hcommit_t *)bmt );                                                            \
}

FD_BMTREE_HOST_API( 20 )
FD_BMTREE_HOST_API( 32 )

/* one tree: its code, and its root to root32 (zeros where it is refused).
   With rows, every leaf's proof as well (leaf k's at rows + k stride): the
   tree's layers are formed one after the other in lay (32 cnt bytes), and
   each is read for the proofs before the next one replaces it. */
static int fd_bmtree_tree_run( unsigned W, unsigned flags, uint32_t cnt, fd_bmtree_gpu_leaf_t const * lf, uint8_t const * blob,
                               unsigned long blob_sz, unsigned long leaf_max, uint8_t * root32,
                               uint8_t * rows, unsigned long stride, uint8_t * lay ) {
  memset( root32, 0, 32 );
  if( !cnt || cnt > leaf_max ) return FD_ED25519_ERR_ARG;
  int nodes = !!( flags & FD_BMTREE_GPU_LEAVES_ARE_NODES );
  for( uint32_t k=0U; k<cnt; k++ ) {
    if( (unsigned long)lf[k].off + (unsigned long)lf[k].sz > blob_sz || (unsigned long)lf[k].off + (unsigned long)lf[k].sz > 0xffffffffUL ) return FD_ED25519_ERR_ARG;
    if( lf[k].sz > FD_BMTREE_GPU_LEAF_SZ_MAX || ( nodes && lf[k].sz != W ) ) return FD_ED25519_ERR_ARG;
  }
  if( rows ) {
    for( uint32_t k=0U; k<cnt; k++ ) {
      uint8_t * leaf = lay + 32UL*k;
      if( nodes ) { memset( leaf, 0, 32 ); memcpy( leaf, blob + lf[k].off, W ); }
      else        fd_bmtree_hleaf( leaf, blob + lf[k].off, lf[k].sz );
    }
    uint32_t cl = cnt;
    for( uint32_t l=0U; cl>1U; l++ ) {
      for( uint32_t k=0U; k<cnt; k++ )
        memcpy( rows + (unsigned long)k*stride + (unsigned long)l*W, lay + 32UL*fd_bmtree_proof_idx( k >> l, cl ), W );
      uint32_t up = ( cl + 1U ) >> 1;
      for( uint32_t j=0U; j<up; j++ )
        fd_bmtree_hmerge( W, lay + 32UL*j, lay + 64UL*j, lay + 32UL*( 2U*j + 1U < cl ? 2U*j + 1U : 2U*j ) );
      cl = up;
    }
    memcpy( root32, lay, W );
    return 0;
  }
  fd_bmtree_hcommit_t c[1] __attribute__((aligned(32)));
  c->leaf_cnt = 0UL;
  for( uint32_t k=0U; k<cnt; k++ ) {
    uint8_t leaf[32];
    if( nodes ) { memset( leaf, 0, 32 ); memcpy( leaf, blob + lf[k].off, W ); }
    else        fd_bmtree_hleaf( leaf, blob + lf[k].off, lf[k].sz );
    fd_bmtree_hpush( W, c, leaf );
  }
  memcpy( root32, fd_bmtree_hfini( W, c ), W );
  return 0;
}

typedef struct {
  unsigned                     W, flags;
  unsigned long                n;
  uint32_t const *             cnt;
  fd_bmtree_gpu_leaf_t const * leaves;
  uint8_t const *              blob;
  unsigned long                blob_sz, leaf_max;
  uint8_t *                    roots;
  int *                        codes;
  unsigned long *              next;
  uint8_t *                    rows;       /* fd_bmtree_proofs_batch: the proof rows, else NULL */
  unsigned long                stride;
  uint8_t *                    lay;        /* lay_sz bytes of layer buffer per worker */
  unsigned long                lay_sz;
  unsigned long *              worker;     /* hands each worker its index */
} fd_bmtree_job_t;

/* trees are taken in runs of this many from a shared cursor */
#define FD_BMTREE_DEAL 8UL

/* the exclusive prefix of cnt[i0, i1) is recomputed from the last run's
   end: runs are dealt in order, so a worker only walks forward */
static void * fd_bmtree_worker( void * arg ) {
  fd_bmtree_job_t * j = (fd_bmtree_job_t *)arg;
  unsigned long at = 0UL, first = 0UL;            /* first = sum of cnt[0, at) */
  uint8_t * lay = j->rows ? j->lay + j->lay_sz * __atomic_fetch_add( j->worker, 1UL, __ATOMIC_RELAXED ) : NULL;
  for(;;) {
    unsigned long i0 = __atomic_fetch_add( j->next, FD_BMTREE_DEAL, __ATOMIC_RELAXED );
    if( i0 >= j->n ) break;
    unsigned long i1 = i0 + FD_BMTREE_DEAL < j->n ? i0 + FD_BMTREE_DEAL : j->n;
    for( ; at<i0; at++ ) first += j->cnt[at];
    for( ; at<i1; at++ ) {
      j->codes[at] = fd_bmtree_tree_run( j->W, j->flags, j->cnt[at], j->leaves + first, j->blob, j->blob_sz, j->leaf_max,
                                         j->roots + 32UL*at, j->rows ? j->rows + first*j->stride : NULL, j->stride, lay );
      first += j->cnt[at];
    }
  }
  return NULL;
}

/* roots_batch, and with emit the proofs too */
static int fd_bmtree_batch( unsigned width, unsigned flags, unsigned long n_trees, uint32_t const * leaf_cnt,
                            fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz, unsigned long leaf_max,
                            void * roots_out, int * codes_out, int emit, void * proofs_out, unsigned long proof_stride, int nthreads ) {
  if( nthreads < 1 || nthreads > 256 ) return FD_ED25519_ERR_ARG;
  if( ( width != 20U && width != 32U ) || ( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) ) return FD_ED25519_ERR_ARG;
  if( n_trees > FD_BMTREE_GPU_LEAVES_MAX || ( n_trees && ( !leaf_cnt || !roots_out || !codes_out ) ) ) return FD_ED25519_ERR_ARG;
  if( emit && ( ( ( (unsigned long)proofs_out | proof_stride ) & 3UL ) || !leaf_max ) ) return FD_ED25519_ERR_ARG;
  if( !n_trees ) return 0;
  unsigned long total = 0UL, widest = 0UL;
  for( unsigned long i=0UL; i<n_trees; i++ ) {
    total += leaf_cnt[i];
    if( leaf_cnt[i] <= leaf_max && leaf_cnt[i] > widest ) widest = leaf_cnt[i];
  }
  if( total > FD_BMTREE_GPU_LEAVES_MAX || ( total && !leaves ) || ( blob_sz && !blob ) ) return FD_ED25519_ERR_ARG;
  unsigned long runs = ( n_trees + FD_BMTREE_DEAL - 1UL ) / FD_BMTREE_DEAL;
  if( (unsigned long)nthreads > runs ) nthreads = (int)runs;
  unsigned long next = 0UL, worker = 0UL;
  fd_bmtree_job_t job = { width, flags, n_trees, leaf_cnt, leaves, (uint8_t const *)blob, blob_sz, leaf_max,
                          (uint8_t *)roots_out, codes_out, &next, NULL, 0UL, NULL, 0UL, &worker };
  if( emit ) {
    if( total && ( !proofs_out || proof_stride < (unsigned long)width * fd_bmtree_depth( (uint32_t)( leaf_max < total ? leaf_max : total ) ) ) )
      return FD_ED25519_ERR_ARG;
    job.lay_sz = 32UL*( widest ? widest : 1UL );
    job.lay    = (uint8_t *)malloc( job.lay_sz * (unsigned long)nthreads );
    if( !job.lay ) return FD_ED25519_ERR_ARG;
    /* no leaves: no row, but the workers take the emit path all the same */
    job.rows = total ? (uint8_t *)proofs_out : job.lay; job.stride = proof_stride;
  }
  pthread_t th[256];
  int started = 0;
  for( int t=1; t<nthreads; t++ ) {
    if( pthread_create( &th[started], NULL, fd_bmtree_worker, &job ) ) break;   /* fewer threads: the others take its share */
    started++;
  }
  fd_bmtree_worker( &job );
  for( int t=0; t<started; t++ ) pthread_join( th[t], NULL );
  free( job.lay );
  return 0;
}

EXPORT int fd_bmtree_roots_batch( unsigned width, unsigned flags, unsigned long n_trees, uint32_t const * leaf_cnt,
                                  fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz,
                                  unsigned long leaf_max, void * roots_out, int * codes_out, int nthreads ) {
  return fd_bmtree_batch( width, flags, n_trees, leaf_cnt, leaves, blob, blob_sz, leaf_max, roots_out, codes_out, 0, NULL, 0UL, nthreads );
}

EXPORT int fd_bmtree_proofs_batch( unsigned width, unsigned flags, unsigned long n_trees, uint32_t const * leaf_cnt,
                                   fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz,
                                   unsigned long leaf_max, void * roots_out, int * codes_out, void * proofs_out,
                                   unsigned long proof_stride, int nthreads ) {
  return fd_bmtree_batch( width, flags, n_trees, leaf_cnt, leaves, blob, blob_sz, leaf_max, roots_out, codes_out, 1, proofs_out,
                          proof_stride, nthreads );
}

/* one proof: its code, and the derived root to root32 (zeros where it is refused) */
static int fd_bmtree_proof_run( unsigned W, unsigned flags, fd_bmtree_gpu_proof_t const * d, uint8_t const * blob, unsigned long blob_sz,
                                unsigned long depth_max, uint8_t * root32 ) {
  int nodes = !!( flags & FD_BMTREE_GPU_LEAVES_ARE_NODES );
  memset( root32, 0, 32 );
  if( !fd_bmtree_proof_ok( W, nodes, blob_sz, (uint32_t)depth_max, FD_BMTREE_GPU_LEAF_SZ_MAX, d->leaf_off, d->leaf_sz, d->proof_off,
                           d->idx, d->leaf_cnt, d->depth, d->expect_off, d->flags ) ) return FD_ED25519_ERR_ARG;
  int words = W == 32U ? 8 : 5;
  uint32_t s[8], p[8];
  if( nodes ) fd_bmtree_load( s, blob + d->leaf_off, words );
  else        fd_bmtree_leaf( s, blob + d->leaf_off, d->leaf_sz );
  for( uint32_t l=0U; l<d->depth; l++ ) {
    int alone = d->leaf_cnt && fd_bmtree_no_sibling( d->idx >> l, fd_bmtree_layer_cnt( d->leaf_cnt, l ) );
    if( !alone ) fd_bmtree_load( p, blob + d->proof_off + (unsigned long)l*W, words );
    fd_bmtree_walk_step( W, s, p, ( d->idx >> l ) & 1U, alone );
  }
  for( int k=words; k<8; k++ ) s[k] = 0U;
  fd_poh_store( root32, s );
  if( !( d->flags & FD_BMTREE_GPU_PROOF_EXPECT ) ) return 0;
  return memcmp( root32, blob + d->expect_off, W ) ? FD_BMTREE_ERR_PROOF : 0;
}

typedef struct {
  unsigned                      W, flags;
  unsigned long                 n;
  fd_bmtree_gpu_proof_t const * proofs;
  uint8_t const *               blob;
  unsigned long                 blob_sz, depth_max;
  uint8_t *                     roots;
  int *                         codes;
  unsigned long *               next;
} fd_bmtree_walk_job_t;

/* proofs are taken in runs of this many from a shared cursor */
#define FD_BMTREE_WALK_DEAL 64UL

static void * fd_bmtree_walk_worker( void * arg ) {
  fd_bmtree_walk_job_t * j = (fd_bmtree_walk_job_t *)arg;
  for(;;) {
    unsigned long i0 = __atomic_fetch_add( j->next, FD_BMTREE_WALK_DEAL, __ATOMIC_RELAXED );
    if( i0 >= j->n ) break;
    unsigned long i1 = i0 + FD_BMTREE_WALK_DEAL < j->n ? i0 + FD_BMTREE_WALK_DEAL : j->n;
    for( unsigned long i=i0; i<i1; i++ )
      j->codes[i] = fd_bmtree_proof_run( j->W, j->flags, j->proofs + i, j->blob, j->blob_sz, j->depth_max, j->roots + 32UL*i );
  }
  return NULL;
}

EXPORT int fd_bmtree_from_proofs_batch( unsigned width, unsigned flags, unsigned long n, fd_bmtree_gpu_proof_t const * proofs,
                                        void const * blob, unsigned long blob_sz, unsigned long depth_max, void * roots_out,
                                        int * codes_out, int nthreads ) {
  if( nthreads < 1 || nthreads > 256 ) return FD_ED25519_ERR_ARG;
  if( ( width != 20U && width != 32U ) || ( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) ) return FD_ED25519_ERR_ARG;
  if( depth_max < 1UL || depth_max > 32UL || n > FD_BMTREE_GPU_LEAVES_MAX ) return FD_ED25519_ERR_ARG;
  if( n && ( !proofs || !roots_out || !codes_out || ( blob_sz && !blob ) ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  unsigned long next = 0UL;
  fd_bmtree_walk_job_t job = { width, flags, n, proofs, (uint8_t const *)blob, blob_sz, depth_max, (uint8_t *)roots_out, codes_out, &next };
  unsigned long runs = ( n + FD_BMTREE_WALK_DEAL - 1UL ) / FD_BMTREE_WALK_DEAL;
  if( (unsigned long)nthreads > runs ) nthreads = (int)runs;
  pthread_t th[256];
  int started = 0;
  for( int t=1; t<nthreads; t++ ) {
    if( pthread_create( &th[started], NULL, fd_bmtree_walk_worker, &job ) ) break;
    started++;
  }
  fd_bmtree_walk_worker( &job );
  for( int t=0; t<started; t++ ) pthread_join( th[t], NULL );
  return 0;
}

/* what the merge launches of the device schedule issue for these shapes:
   layer by layer, the parents of all trees dense, one lane each */
EXPORT unsigned long fd_bmtree_gpu_merge_passes( unsigned width, unsigned long n_trees, uint32_t const * leaf_cnt ) {
  if( ( width != 20U && width != 32U ) || ( n_trees && !leaf_cnt ) ) return 0UL;
  unsigned long passes = 0UL;
  for( unsigned l=1U; l<=32U; l++ ) {
    unsigned long lanes = 0UL;
    for( unsigned long i=0UL; i<n_trees; i++ ) {
      unsigned long c = ( (unsigned long)leaf_cnt[i] + ( 1UL << (l-1U) ) - 1UL ) >> (l-1U);   /* nodes of layer l-1 */
      if( c > 1UL ) lanes += ( c + 1UL ) >> 1;
    }
    if( !lanes ) break;
    passes += ( ( lanes + 63UL ) >> 6 ) * ( width == 32U ? 2UL : 1UL );
  }
  return passes;
}
