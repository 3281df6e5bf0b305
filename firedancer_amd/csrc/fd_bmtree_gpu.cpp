/* fd_bmtree_gpu.cpp -- host side of the Merkle tree device path
   (include/fd_bmtree_gpu.h; the kernels are fd_bmtree_gpu_kernels.hip).

   It is a side unit of the engine (fd_ed25519_gpu_unit.h), with nothing of
   its own beyond the common state.

   The device call queues a fixed sequence (fd_bmtree_gpu_launch) whose
   length comes from the shapes alone.  The packed call stages the inputs
   through pinned memory, runs the device call on the unit's stream and
   waits for it within the engine's timeout. */

#include <string.h>
#include "fd_ed25519_gpu_unit.h"
#include "fd_bmtree_gpu_private.h"

#define FD_EXPORT extern "C" __attribute__((visibility("default")))

/* the unit's scratch */
enum { FD_BMTREE_D_BUF,    /* first | leaves | blob | roots | codes | proof rows | work; from proofs: descriptors | blob | roots | codes */
       FD_BMTREE_H_IN,     /* pinned: first | leaves | blob; from proofs: descriptors | blob */
       FD_BMTREE_H_OUT };  /* pinned: roots | codes | proof rows */

static inline fd_gpu_unit * fd_bmtree_unit( fd_ed25519_gpu_t * gpu ) {
  return fd_gpu_unit_get<fd_gpu_unit>( gpu, FD_GPU_UNIT_BMTREE, "bmtree" );
}

fd_bmtree_staged_t fd_bmtree_gpu_stage( uint8_t * h, unsigned long n, uint32_t const * leaf_cnt, unsigned long n_leaves,
                                        fd_bmtree_gpu_leaf_t const * leaves, void const * blob, unsigned long blob_sz ) {
  fd_bmtree_staged_t sz = { fd_gpu_r16( 4UL*( n + 1UL ) ), fd_gpu_r16( 8UL*n_leaves ), fd_gpu_r16( blob_sz ) };
  if( !h ) return sz;
  uint32_t * h_first = (uint32_t *)h;
  unsigned long run = 0UL;
  for( unsigned long i=0UL; i<n; i++ ) { h_first[i] = (uint32_t)run; run += leaf_cnt[i]; }
  h_first[n] = (uint32_t)run;
  if( n_leaves ) memcpy( h + sz.first_sz, leaves, 8UL*n_leaves );
  if( blob_sz  ) memcpy( h + sz.first_sz + sz.leaf_sz, blob, blob_sz );
  return sz;
}

FD_EXPORT unsigned long fd_bmtree_gpu_work_sz( unsigned long n_trees, unsigned long n_leaves ) {
  if( n_trees > FD_BMTREE_GPU_LEAVES_MAX || n_leaves > FD_BMTREE_GPU_LEAVES_MAX ) return 0UL;
  fd_bmtree_plan_t p;
  memset( &p, 0, sizeof(p) );
  p.T = (uint32_t)n_trees; p.N = (uint32_t)n_leaves;
  return fd_bmtree_plan_layout( &p, NULL );
}

static inline int fd_bmtree_args_ok( unsigned width, unsigned flags, unsigned allowed, unsigned long n_trees, unsigned long blob_sz,
                                     unsigned long leaf_max ) {
  return ( width == 20U || width == 32U ) && !( flags & ~allowed ) && n_trees <= FD_BMTREE_GPU_LEAVES_MAX &&
         blob_sz <= 0xffffffffUL && leaf_max >= 1UL;
}

/* the emit calls' proof rows: stride and base multiples of 4, the stride
   at least the deepest proof the count rules allow, a base where there are
   leaves */
static inline int fd_bmtree_rows_ok( unsigned width, unsigned long n_leaves, unsigned long leaf_max, void const * proofs, unsigned long stride ) {
  if( ( (uintptr_t)proofs | stride ) & 3UL ) return 0;
  if( !n_leaves ) return 1;
  return proofs && stride >= (unsigned long)width * fd_bmtree_ceil_log2( leaf_max < n_leaves ? leaf_max : n_leaves );
}

/* the device-resident calls: roots, and with emit the proof rows */
static int fd_bmtree_dev_call( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees, uint32_t const * d_first,
                               unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves, void const * d_blob, unsigned long blob_sz,
                               unsigned long leaf_max, void * d_roots, unsigned long root_stride, int emit, void * d_proofs,
                               unsigned long proof_stride, int * d_codes, void * d_work, void * stream ) {
  if( !fd_bmtree_args_ok( width, flags, FD_BMTREE_GPU_LEAVES_ARE_NODES | FD_BMTREE_GPU_SKIP_EMPTY, n_trees, blob_sz, leaf_max ) ) return FD_ED25519_ERR_ARG;
  if( n_leaves > FD_BMTREE_GPU_LEAVES_MAX ) return FD_ED25519_ERR_ARG;
  if( n_trees && ( !d_first || !d_roots || !d_codes || !d_work ) ) return FD_ED25519_ERR_ARG;
  if( n_leaves && ( !d_leaves || ( blob_sz && !d_blob ) ) ) return FD_ED25519_ERR_ARG;
  if( ( (uintptr_t)d_work & 15UL ) || ( ( (uintptr_t)d_roots | root_stride | (uintptr_t)d_first | (uintptr_t)d_leaves | (uintptr_t)d_codes ) & 3UL ) ||
      ( n_trees && root_stride < 32UL ) ) return FD_ED25519_ERR_ARG;
  if( emit && !fd_bmtree_rows_ok( width, n_leaves, leaf_max, d_proofs, proof_stride ) ) return FD_ED25519_ERR_ARG;
  if( !n_trees ) return 0;
  fd_gpu_unit * c = fd_bmtree_unit( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "hipSetDevice", e );
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, width, flags, n_trees, n_leaves, blob_sz, leaf_max, (uint8_t *)d_work, lanes );
  p.first = d_first; p.leaves = d_leaves; p.blob = (uint8_t const *)d_blob;
  p.roots = (uint8_t *)d_roots; p.root_stride = root_stride; p.codes = (int32_t *)d_codes;
  if( emit ) { p.proofs = (uint8_t *)d_proofs; p.proof_stride = proof_stride; }
  e = fd_bmtree_gpu_launch( &p, lanes, stream ? (hipStream_t)stream : c->stream );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "bmtree launch", e );
  return 0;
}

extern "C" int fd_bmtree_gpu_roots_dev_flags( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                              uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                              void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                              unsigned long root_stride, int * d_codes, void * d_work, void * stream ) {
  return fd_bmtree_dev_call( gpu, width, flags, n_trees, d_first, n_leaves, d_leaves, d_blob, blob_sz, leaf_max, d_roots, root_stride,
                             0, NULL, 0UL, d_codes, d_work, stream );
}

FD_EXPORT int fd_bmtree_gpu_roots_dev( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                       uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                       void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                       unsigned long root_stride, int * d_codes, void * d_work, void * stream ) {
  if( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) return FD_ED25519_ERR_ARG;
  return fd_bmtree_dev_call( gpu, width, flags, n_trees, d_first, n_leaves, d_leaves, d_blob, blob_sz, leaf_max, d_roots, root_stride,
                             0, NULL, 0UL, d_codes, d_work, stream );
}

FD_EXPORT int fd_bmtree_gpu_proofs_dev( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                        uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                        void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                        unsigned long root_stride, void * d_proofs, unsigned long proof_stride, int * d_codes,
                                        void * d_work, void * stream ) {
  if( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) return FD_ED25519_ERR_ARG;
  return fd_bmtree_dev_call( gpu, width, flags, n_trees, d_first, n_leaves, d_leaves, d_blob, blob_sz, leaf_max, d_roots, root_stride,
                             1, d_proofs, proof_stride, d_codes, d_work, stream );
}

/* the packed calls: roots and codes, and with emit the proof rows, which
   the device writes packed (W L bytes a leaf) behind the codes and the host
   copies to the caller's rows, W D bytes for each leaf of a tree that is
   not refused */
static int fd_bmtree_packed_call( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                  uint32_t const * leaf_cnt, fd_bmtree_gpu_leaf_t const * leaves, void const * blob,
                                  unsigned long blob_sz, unsigned long leaf_max, void * roots_out, int * codes_out,
                                  int emit, void * proofs_out, unsigned long proof_stride ) {
  if( !fd_bmtree_args_ok( width, flags, FD_BMTREE_GPU_LEAVES_ARE_NODES, n_trees, blob_sz, leaf_max ) ) return FD_ED25519_ERR_ARG;
  if( n_trees && ( !leaf_cnt || !roots_out || !codes_out ) ) return FD_ED25519_ERR_ARG;
  if( emit && ( ( (uintptr_t)proofs_out | proof_stride ) & 3UL ) ) return FD_ED25519_ERR_ARG;
  if( !n_trees ) return 0;
  unsigned long n_leaves = 0UL;
  for( unsigned long i=0UL; i<n_trees; i++ ) n_leaves += leaf_cnt[i];
  if( n_leaves > FD_BMTREE_GPU_LEAVES_MAX || ( n_leaves && !leaves ) || ( blob_sz && !blob ) ) return FD_ED25519_ERR_ARG;
  if( emit && !fd_bmtree_rows_ok( width, n_leaves, leaf_max, proofs_out, proof_stride ) ) return FD_ED25519_ERR_ARG;
  fd_gpu_unit * c = fd_bmtree_unit( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );

  int err = fd_gpu_unit_begin( c );
  if( err ) return err;
  fd_bmtree_staged_t in = fd_bmtree_gpu_stage( NULL, n_trees, leaf_cnt, n_leaves, leaves, blob, blob_sz );
  unsigned long first_sz = in.first_sz, leaf_sz = in.leaf_sz, in_sz = first_sz + leaf_sz + in.blob_sz;
  unsigned long row_sz   = emit ? (unsigned long)width * fd_bmtree_ceil_log2( leaf_max < n_leaves ? leaf_max : n_leaves ) : 0UL;
  unsigned long root_sz  = 32UL*n_trees, code_sz = fd_gpu_r16( 4UL*n_trees ), rows_sz = fd_gpu_r16( row_sz*n_leaves );
  unsigned long out_sz   = root_sz + code_sz + rows_sz;
  unsigned long work_sz  = fd_bmtree_gpu_work_sz( n_trees, n_leaves );
  if( (err = fd_gpu_unit_grow( c, FD_BMTREE_D_BUF, 0, in_sz + out_sz + work_sz )) ||
      (err = fd_gpu_unit_grow( c, FD_BMTREE_H_IN,  1, in_sz )) ||
      (err = fd_gpu_unit_grow( c, FD_BMTREE_H_OUT, 1, out_sz )) ) return err;
  uint8_t * h_in = c->buf[FD_BMTREE_H_IN].p, * h_out = c->buf[FD_BMTREE_H_OUT].p;
  fd_bmtree_gpu_stage( h_in, n_trees, leaf_cnt, n_leaves, leaves, blob, blob_sz );

  uint8_t * d_in = c->buf[FD_BMTREE_D_BUF].p, * d_out = d_in + in_sz, * d_work = d_out + out_sz;
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, width, flags, n_trees, n_leaves, blob_sz, leaf_max, d_work, lanes );
  p.first = (uint32_t const *)d_in; p.leaves = (fd_bmtree_gpu_leaf_t const *)( d_in + first_sz ); p.blob = d_in + first_sz + leaf_sz;
  p.roots = d_out; p.root_stride = 32UL; p.codes = (int32_t *)( d_out + root_sz );
  if( emit ) { p.proofs = d_out + root_sz + code_sz; p.proof_stride = row_sz; }
  /* the host knows the counts: the lanes of the trees the count rules keep */
  for( uint32_t l=0U; l<p.L; l++ ) lanes[l] = 0U;
  for( unsigned long i=0UL; i<n_trees; i++ ) {
    unsigned long cc = leaf_cnt[i] <= leaf_max ? leaf_cnt[i] : 0UL;
    for( uint32_t l=0U; l<p.L && cc>1UL; l++ ) { cc = ( cc + 1UL ) >> 1; lanes[l] += (uint32_t)cc; }
  }

  hipError_t e = hipMemcpyAsync( d_in, h_in, in_sz, hipMemcpyHostToDevice, c->stream );
  if( e == hipSuccess ) e = fd_bmtree_gpu_launch( &p, lanes, c->stream );
  if( e == hipSuccess ) e = hipMemcpyAsync( h_out, d_out, out_sz, hipMemcpyDeviceToHost, c->stream );
  if( (err = fd_gpu_unit_finish( c, e )) ) return err;

  memcpy( roots_out, h_out, root_sz );
  memcpy( codes_out, h_out + root_sz, 4UL*n_trees );
  if( emit ) {
    uint8_t const * rows = h_out + root_sz + code_sz;
    unsigned long k = 0UL;
    for( unsigned long i=0UL; i<n_trees; k+=leaf_cnt[i], i++ ) {
      unsigned long take = (unsigned long)width * fd_bmtree_ceil_log2( leaf_cnt[i] );
      if( codes_out[i] || !take ) continue;
      for( unsigned long j=k; j<k+leaf_cnt[i]; j++ ) memcpy( (uint8_t *)proofs_out + j*proof_stride, rows + j*row_sz, take );
    }
  }
  return 0;
}

FD_EXPORT int fd_bmtree_gpu_roots_packed( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                          uint32_t const * leaf_cnt, fd_bmtree_gpu_leaf_t const * leaves, void const * blob,
                                          unsigned long blob_sz, unsigned long leaf_max, void * roots_out, int * codes_out ) {
  return fd_bmtree_packed_call( gpu, width, flags, n_trees, leaf_cnt, leaves, blob, blob_sz, leaf_max, roots_out, codes_out, 0, NULL, 0UL );
}

FD_EXPORT int fd_bmtree_gpu_proofs_packed( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                           uint32_t const * leaf_cnt, fd_bmtree_gpu_leaf_t const * leaves, void const * blob,
                                           unsigned long blob_sz, unsigned long leaf_max, void * roots_out, int * codes_out,
                                           void * proofs_out, unsigned long proof_stride ) {
  return fd_bmtree_packed_call( gpu, width, flags, n_trees, leaf_cnt, leaves, blob, blob_sz, leaf_max, roots_out, codes_out, 1,
                                proofs_out, proof_stride );
}

/* from proofs: the arguments both device calls share */
static inline int fd_bmtree_walk_args_ok( unsigned width, unsigned flags, unsigned long n, unsigned long blob_sz, unsigned long depth_max ) {
  return ( width == 20U || width == 32U ) && !( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) && n <= FD_BMTREE_GPU_LEAVES_MAX &&
         blob_sz <= 0xffffffffUL && depth_max >= 1UL && depth_max <= 32UL;
}

static inline void fd_bmtree_walk_plan_make( fd_bmtree_walk_plan_t * p, unsigned width, unsigned flags, unsigned long n, unsigned long blob_sz,
                                             unsigned long depth_max ) {
  memset( p, 0, sizeof(*p) );
  p->width = width; p->flags = flags; p->n = (uint32_t)n; p->blob_sz = (uint32_t)blob_sz; p->depth_max = (uint32_t)depth_max;
}

FD_EXPORT int fd_bmtree_gpu_from_proofs_dev( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n,
                                             fd_bmtree_gpu_proof_t const * d_proofs, void const * d_blob, unsigned long blob_sz,
                                             unsigned long depth_max, void * d_roots, unsigned long root_stride, int * d_codes,
                                             void * stream ) {
  if( !fd_bmtree_walk_args_ok( width, flags, n, blob_sz, depth_max ) ) return FD_ED25519_ERR_ARG;
  if( n && ( !d_proofs || !d_roots || !d_codes || ( blob_sz && !d_blob ) ) ) return FD_ED25519_ERR_ARG;
  if( ( ( (uintptr_t)d_roots | root_stride | (uintptr_t)d_proofs | (uintptr_t)d_codes ) & 3UL ) || ( n && root_stride < 32UL ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_gpu_unit * c = fd_bmtree_unit( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "hipSetDevice", e );
  fd_bmtree_walk_plan_t p;
  fd_bmtree_walk_plan_make( &p, width, flags, n, blob_sz, depth_max );
  p.desc = d_proofs; p.blob = (uint8_t const *)d_blob;
  p.roots = (uint8_t *)d_roots; p.root_stride = root_stride; p.codes = (int32_t *)d_codes;
  e = fd_bmtree_gpu_walk_launch( &p, stream ? (hipStream_t)stream : c->stream );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "bmtree launch", e );
  return 0;
}

FD_EXPORT int fd_bmtree_gpu_from_proofs_packed( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n,
                                                fd_bmtree_gpu_proof_t const * proofs, void const * blob, unsigned long blob_sz,
                                                unsigned long depth_max, void * roots_out, int * codes_out ) {
  if( !fd_bmtree_walk_args_ok( width, flags, n, blob_sz, depth_max ) ) return FD_ED25519_ERR_ARG;
  if( n && ( !proofs || !roots_out || !codes_out || ( blob_sz && !blob ) ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_gpu_unit * c = fd_bmtree_unit( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );

  int err = fd_gpu_unit_begin( c );
  if( err ) return err;
  unsigned long desc_sz = sizeof(fd_bmtree_gpu_proof_t)*n, in_sz = desc_sz + fd_gpu_r16( blob_sz );
  unsigned long root_sz = 32UL*n, out_sz = root_sz + fd_gpu_r16( 4UL*n );
  if( (err = fd_gpu_unit_grow( c, FD_BMTREE_D_BUF, 0, in_sz + out_sz )) ||
      (err = fd_gpu_unit_grow( c, FD_BMTREE_H_IN,  1, in_sz )) ||
      (err = fd_gpu_unit_grow( c, FD_BMTREE_H_OUT, 1, out_sz )) ) return err;
  uint8_t * h_in = c->buf[FD_BMTREE_H_IN].p, * h_out = c->buf[FD_BMTREE_H_OUT].p;
  memcpy( h_in, proofs, desc_sz );
  if( blob_sz ) memcpy( h_in + desc_sz, blob, blob_sz );

  uint8_t * d_in = c->buf[FD_BMTREE_D_BUF].p, * d_out = d_in + in_sz;
  fd_bmtree_walk_plan_t p;
  fd_bmtree_walk_plan_make( &p, width, flags, n, blob_sz, depth_max );
  p.desc = (fd_bmtree_gpu_proof_t const *)d_in; p.blob = d_in + desc_sz;
  p.roots = d_out; p.root_stride = 32UL; p.codes = (int32_t *)( d_out + root_sz );

  hipError_t e = hipMemcpyAsync( d_in, h_in, in_sz, hipMemcpyHostToDevice, c->stream );
  if( e == hipSuccess ) e = fd_bmtree_gpu_walk_launch( &p, c->stream );
  if( e == hipSuccess ) e = hipMemcpyAsync( h_out, d_out, out_sz, hipMemcpyDeviceToHost, c->stream );
  if( (err = fd_gpu_unit_finish( c, e )) ) return err;

  memcpy( roots_out, h_out, root_sz );
  memcpy( codes_out, h_out + root_sz, 4UL*n );
  return 0;
}
