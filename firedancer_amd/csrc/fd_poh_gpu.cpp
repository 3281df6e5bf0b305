/* fd_poh_gpu.cpp -- host side of the Proof-of-History device path
   (include/fd_poh_gpu.h; the kernel is fd_k_poh, fd_poh_gpu_kernels.hip).

   It is a side unit of the engine (fd_ed25519_gpu_unit.h); its own state
   is the chunk and the lane-order switch.

   The packed call orders the lanes by n descending.  Each wave then holds
   chains of about one length, the long chains start in the first launch,
   and launch j is given only the prefix of lanes with n > j C: the lanes
   past it are done and would cost a load each.

   The entries calls take an entry's leaves instead of its mixin: ahead of
   the first fd_k_poh launch, on the same stream, the tree launcher
   (fd_bmtree_gpu_private.h) writes each entry's bmtree32 root into the
   mixin field of its device copy, and a gate kernel marks the entries
   whose leaves cannot be used so that fd_k_poh refuses them unhashed. */

#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>
#include "fd_ed25519_gpu_unit.h"
#include "fd_poh_gpu_private.h"
#include "fd_bmtree_gpu_private.h"

#define FD_EXPORT extern "C" __attribute__((visibility("default")))

#define FD_POH_N_MAX      0x7fffffffUL   /* entries per call */
#define FD_POH_CHUNK_MAX  (1UL<<24)
#define FD_POH_ENT_SZ     sizeof(fd_poh_gpu_entry_t)
#define FD_POH_ROW_SZ     (4UL*FD_POH_ROW_WORDS)

struct __attribute__((visibility("hidden"))) fd_poh_ctx : fd_gpu_unit {
  unsigned long chunk = FD_POH_GPU_CHUNK_DEFAULT;   /* hashes per lane per launch */
  int           nosort = 0;  /* experiments (fd_poh_gpu_debug_set_sort): the packed call keeps the caller's lane order */
};

/* the unit's scratch */
enum { FD_POH_D_BUF,     /* entries | order | codes | states | work rows, each for the call's n rounded up to 4 */
       FD_POH_H_IN,      /* pinned: entries | order */
       FD_POH_H_OUT,     /* pinned: codes | states */
       FD_POH_D_TREE,    /* the entries call's trees: first | leaves | blob | tree codes | tree work */
       FD_POH_H_TREE };  /* pinned: first | leaves | blob */

static inline fd_poh_ctx * fd_poh_ctx_get( fd_ed25519_gpu_t * gpu ) {
  return fd_gpu_unit_get<fd_poh_ctx>( gpu, FD_GPU_UNIT_POH, "poh" );
}

/* the leaves of fd_poh_gpu_verify_entries_packed */
struct fd_poh_trees {
  uint32_t const *             leaf_cnt;
  fd_bmtree_gpu_leaf_t const * leaves;
  void const *                 blob;
  unsigned long                blob_sz, leaf_max, n_leaves;
};

static inline unsigned long fd_poh_r4( unsigned long n ) { return ( n + 3UL ) & ~3UL; }

static inline int fd_poh_entry_ok( fd_poh_gpu_entry_t const * e, unsigned long n_max ) {
  return !( e->flags & ~FD_POH_GPU_MIXIN ) && !e->_pad && e->n <= n_max;
}

/* launches for chains of up to max_n hashes at C per launch: at least one
   (it writes the codes of the n = 0 and the refused entries) */
static inline unsigned long fd_poh_launches( unsigned long max_n, unsigned long C ) {
  unsigned long l = max_n / C + (unsigned long)( max_n % C != 0UL );
  return l ? l : 1UL;
}

FD_EXPORT unsigned long fd_poh_gpu_work_sz( unsigned long n ) { return ( n ? n : 1UL ) * FD_POH_ROW_SZ; }

FD_EXPORT int fd_poh_gpu_debug_set_chunk( fd_ed25519_gpu_t * gpu, unsigned long C ) {
  if( C > FD_POH_CHUNK_MAX ) return FD_ED25519_ERR_ARG;
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );
  c->chunk = C ? C : FD_POH_GPU_CHUNK_DEFAULT;
  return 0;
}

FD_EXPORT int fd_poh_gpu_debug_set_sort( fd_ed25519_gpu_t * gpu, int on ) {
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );
  c->nosort = !on;
  return 0;
}

FD_EXPORT unsigned long fd_poh_gpu_chunk( fd_ed25519_gpu_t * gpu ) {
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return 0UL;
  std::lock_guard<std::mutex> guard( c->lock );
  return c->chunk;
}

/* tr NULL: fd_poh_gpu_verify_packed; else the entries call, its arguments checked */
static int fd_poh_packed( fd_ed25519_gpu_t * gpu, unsigned long n, fd_poh_gpu_entry_t const * entries,
                          unsigned long n_max, int * out, void * state_out_opt, fd_poh_trees const * tr ) {
  if( n > FD_POH_N_MAX || ( n && ( !entries || !out ) ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );
  unsigned long C = c->chunk;

  /* lane order: n descending, entries of one n in the caller's order;
     refused entries count as n = 0 (the first launch writes their code).
     Chains below 2^32 hashes sort as one 64-bit key each. */
  unsigned long max_n = 0UL;
  auto ok = [&]( unsigned long i ) {    /* what is known here of what the first launch will refuse */
    return fd_poh_entry_ok( entries + i, n_max ) && !( tr && tr->leaf_cnt[i] && !( entries[i].flags & FD_POH_GPU_MIXIN ) );
  };
  for( unsigned long i=0; i<n; i++ ) if( ok( i ) && entries[i].n > max_n ) max_n = entries[i].n;
  unsigned long launches = fd_poh_launches( max_n, C );
  if( launches > FD_POH_GPU_LAUNCH_MAX ) return FD_ED25519_ERR_ARG;
  std::vector<uint32_t> order( n );
  std::vector<uint64_t> len( n );       /* len[i]: hashes of lane i */
  if( c->nosort ) {                     /* the A/B's other side: every launch covers every lane */
    for( unsigned long i=0; i<n; i++ ) { order[i] = (uint32_t)i; len[i] = max_n; }
  } else if( max_n <= 0xffffffffUL ) {
    std::vector<uint64_t> key( n );
    for( unsigned long i=0; i<n; i++ )
      key[i] = ( ( ok( i ) ? entries[i].n : 0UL ) << 32 ) | ( 0xffffffffUL - i );
    std::sort( key.begin(), key.end(), std::greater<uint64_t>() );
    for( unsigned long i=0; i<n; i++ ) { order[i] = (uint32_t)( 0xffffffffUL - ( key[i] & 0xffffffffUL ) ); len[i] = key[i] >> 32; }
  } else {
    for( unsigned long i=0; i<n; i++ ) order[i] = (uint32_t)i;
    auto eff = [&]( uint32_t i ) { return ok( i ) ? entries[i].n : 0UL; };
    std::stable_sort( order.begin(), order.end(), [&]( uint32_t a, uint32_t b ) { return eff( a ) > eff( b ); } );
    for( unsigned long i=0; i<n; i++ ) len[i] = eff( order[i] );
  }

  int err = fd_gpu_unit_begin( c );
  if( err ) return err;
  unsigned long n4     = fd_poh_r4( n );
  unsigned long in_sz  = n4 * ( FD_POH_ENT_SZ + 4UL );
  unsigned long out_sz = n4 * ( state_out_opt ? 36UL : 4UL );
  if( (err = fd_gpu_unit_grow( c, FD_POH_D_BUF, 0, n4 * ( FD_POH_ENT_SZ + 4UL + 4UL + 32UL + FD_POH_ROW_SZ ) )) ||
      (err = fd_gpu_unit_grow( c, FD_POH_H_IN,  1, in_sz )) ||
      (err = fd_gpu_unit_grow( c, FD_POH_H_OUT, 1, n4 * 36UL )) ) return err;
  uint8_t * h_in = c->buf[FD_POH_H_IN].p, * h_out = c->buf[FD_POH_H_OUT].p;
  uint8_t * d_ent   = c->buf[FD_POH_D_BUF].p;
  uint8_t * d_order = d_ent   + n4 * FD_POH_ENT_SZ;
  uint8_t * d_out   = d_order + n4 * 4UL;
  uint8_t * d_state = d_out   + n4 * 4UL;
  uint8_t * d_work  = d_state + n4 * 32UL;
  memcpy( h_in, entries, n * FD_POH_ENT_SZ );
  memcpy( h_in + n4 * FD_POH_ENT_SZ, order.data(), n * 4UL );

  /* the trees' inputs, staged like the entries */
  unsigned long first_sz = 0UL, leaf_sz = 0UL, t_in_sz = 0UL, tcode_sz = fd_gpu_r16( 4UL*n );
  uint8_t * d_tree = NULL;
  if( tr && tr->n_leaves ) {
    fd_bmtree_staged_t in = fd_bmtree_gpu_stage( NULL, n, tr->leaf_cnt, tr->n_leaves, tr->leaves, tr->blob, tr->blob_sz );
    first_sz = in.first_sz; leaf_sz = in.leaf_sz; t_in_sz = first_sz + leaf_sz + in.blob_sz;
    if( (err = fd_gpu_unit_grow( c, FD_POH_D_TREE, 0, t_in_sz + tcode_sz + fd_bmtree_gpu_work_sz( n, tr->n_leaves ) )) ||
        (err = fd_gpu_unit_grow( c, FD_POH_H_TREE, 1, t_in_sz )) ) return err;
    d_tree = c->buf[FD_POH_D_TREE].p;
    fd_bmtree_gpu_stage( c->buf[FD_POH_H_TREE].p, n, tr->leaf_cnt, tr->n_leaves, tr->leaves, tr->blob, tr->blob_sz );
  }

  hipError_t e = hipMemcpyAsync( d_ent, h_in, in_sz, hipMemcpyHostToDevice, c->stream );
  if( e == hipSuccess && t_in_sz ) e = hipMemcpyAsync( d_tree, c->buf[FD_POH_H_TREE].p, t_in_sz, hipMemcpyHostToDevice, c->stream );
  if( e == hipSuccess && t_in_sz ) {    /* roots into the mixins, then the gate, ahead of the first chain launch */
    uint8_t * d_tcodes = d_tree + t_in_sz;
    int r = fd_bmtree_gpu_roots_dev_flags( c->gpu, 32U, FD_BMTREE_GPU_SKIP_EMPTY, n, (uint32_t const *)d_tree, tr->n_leaves,
                                           (fd_bmtree_gpu_leaf_t const *)( d_tree + first_sz ), d_tree + first_sz + leaf_sz,
                                           tr->blob_sz, tr->leaf_max, d_ent + 32UL, FD_POH_ENT_SZ, (int *)d_tcodes, d_tcodes + tcode_sz,
                                           c->stream );
    if( r ) e = hipErrorLaunchFailure;
    else    e = fd_bmtree_gpu_poh_gate_launch( (uint32_t)n, (uint32_t const *)d_tree, (int32_t const *)d_tcodes,
                                               (fd_poh_gpu_entry_t *)d_ent, c->stream );
  }
  unsigned long lanes = n;
  for( unsigned long j=0; j<launches && e == hipSuccess; j++ ) {
    if( j ) {                           /* the lanes with more than j C hashes */
      while( lanes && len[lanes-1UL] <= j * C ) lanes--;
      if( !lanes ) break;
    }
    e = fd_poh_gpu_launch( (uint32_t)lanes, j == 0UL, (uint32_t)C, n_max, (fd_poh_gpu_entry_t const *)d_ent, (uint32_t const *)d_order,
                           (uint32_t *)d_work, (int32_t *)d_out, state_out_opt ? d_state : NULL, c->stream );
  }
  if( e == hipSuccess ) e = hipMemcpyAsync( h_out, d_out, out_sz, hipMemcpyDeviceToHost, c->stream );
  if( (err = fd_gpu_unit_finish( c, e )) ) return err;

  memcpy( out, h_out, n * 4UL );
  if( state_out_opt ) memcpy( state_out_opt, h_out + n4 * 4UL, n * 32UL );
  return 0;
}

FD_EXPORT int fd_poh_gpu_verify_packed( fd_ed25519_gpu_t * gpu, unsigned long n, fd_poh_gpu_entry_t const * entries,
                                        unsigned long n_max, int * out, void * state_out_opt ) {
  return fd_poh_packed( gpu, n, entries, n_max, out, state_out_opt, NULL );
}

FD_EXPORT int fd_poh_gpu_verify_entries_packed( fd_ed25519_gpu_t * gpu, unsigned long n, fd_poh_gpu_entry_t const * entries,
                                                unsigned long n_max, int * out, void * state_out_opt, uint32_t const * leaf_cnt,
                                                fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz,
                                                unsigned long leaf_max ) {
  if( n > FD_POH_N_MAX || ( n && ( !entries || !out || !leaf_cnt ) ) ) return FD_ED25519_ERR_ARG;
  if( blob_sz > 0xffffffffUL || !leaf_max ) return FD_ED25519_ERR_ARG;
  fd_poh_trees tr = { leaf_cnt, leaves, blob, blob_sz, leaf_max, 0UL };
  for( unsigned long i=0; i<n; i++ ) tr.n_leaves += leaf_cnt[i];
  if( tr.n_leaves > FD_BMTREE_GPU_LEAVES_MAX || ( tr.n_leaves && !leaves ) || ( blob_sz && !blob ) ) return FD_ED25519_ERR_ARG;
  return fd_poh_packed( gpu, n, entries, n_max, out, state_out_opt, &tr );
}

FD_EXPORT unsigned long fd_poh_gpu_entries_work_sz( unsigned long n, unsigned long n_leaves ) {
  unsigned long w = fd_bmtree_gpu_work_sz( n, n_leaves );
  return w ? fd_gpu_r16( 4UL*( n ? n : 1UL ) ) + w : 0UL;
}

FD_EXPORT int fd_poh_gpu_verify_entries_dev( fd_ed25519_gpu_t * gpu, unsigned long n, fd_poh_gpu_entry_t * d_entries, unsigned long n_max,
                                             int * d_out, void * d_state_out_opt, void * d_work, uint32_t const * d_first,
                                             unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves, void const * d_blob,
                                             unsigned long blob_sz, unsigned long leaf_max, void * d_tree_work, void * stream ) {
  if( n > FD_POH_N_MAX || ( n && ( !d_entries || !d_out || !d_work || !d_first || !d_tree_work ) ) ) return FD_ED25519_ERR_ARG;
  if( ( (uintptr_t)d_work | (uintptr_t)d_state_out_opt | (uintptr_t)d_tree_work ) & 15UL ) return FD_ED25519_ERR_ARG;
  if( ( (uintptr_t)d_entries & 7UL ) || blob_sz > 0xffffffffUL || !leaf_max || n_leaves > FD_BMTREE_GPU_LEAVES_MAX ) return FD_ED25519_ERR_ARG;
  if( n_leaves && ( !d_leaves || ( blob_sz && !d_blob ) ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  { std::lock_guard<std::mutex> guard( c->lock );
    if( fd_poh_launches( n_max, c->chunk ) > FD_POH_GPU_LAUNCH_MAX ) return FD_ED25519_ERR_ARG; }   /* before anything is queued */
  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "hipSetDevice", e );
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if( n_leaves ) {
    uint8_t * d_tcodes = (uint8_t *)d_tree_work;
    int r = fd_bmtree_gpu_roots_dev_flags( c->gpu, 32U, FD_BMTREE_GPU_SKIP_EMPTY, n, d_first, n_leaves, d_leaves, d_blob, blob_sz, leaf_max,
                                           (uint8_t *)d_entries + 32UL, FD_POH_ENT_SZ, (int *)d_tcodes, d_tcodes + fd_gpu_r16( 4UL*n ), st );
    if( r ) return r;
    e = fd_bmtree_gpu_poh_gate_launch( (uint32_t)n, d_first, (int32_t const *)d_tcodes, d_entries, st );
    if( e != hipSuccess ) return fd_gpu_unit_fail( "poh gate launch", e );
  }
  return fd_poh_gpu_verify_dev( c->gpu, n, d_entries, n_max, d_out, d_state_out_opt, d_work, st );
}

FD_EXPORT int fd_poh_gpu_verify_dev( fd_ed25519_gpu_t * gpu, unsigned long n, fd_poh_gpu_entry_t const * d_entries, unsigned long n_max,
                                     int * d_out, void * d_state_out_opt, void * d_work, void * stream ) {
  if( n > FD_POH_N_MAX || ( n && ( !d_entries || !d_out || !d_work ) ) ) return FD_ED25519_ERR_ARG;
  if( ( (uintptr_t)d_work | (uintptr_t)d_state_out_opt ) & 15UL ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_poh_ctx * c = fd_poh_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  unsigned long C;
  { std::lock_guard<std::mutex> guard( c->lock ); C = c->chunk; }
  unsigned long launches = fd_poh_launches( n_max, C );
  if( launches > FD_POH_GPU_LAUNCH_MAX ) return FD_ED25519_ERR_ARG;
  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "hipSetDevice", e );
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  for( unsigned long j=0; j<launches; j++ ) {
    e = fd_poh_gpu_launch( (uint32_t)n, j == 0UL, (uint32_t)C, n_max, d_entries, NULL, (uint32_t *)d_work, (int32_t *)d_out,
                           (uint8_t *)d_state_out_opt, st );
    if( e != hipSuccess ) return fd_gpu_unit_fail( "poh launch", e );
  }
  return 0;
}
