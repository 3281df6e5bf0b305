/* fd_bmtree_gpu.cpp -- host side of the Merkle tree device path
   (include/fd_bmtree_gpu.h; the kernels are fd_bmtree_gpu_kernels.hip).

   It hangs off the engine through one slot (fd_ed25519_gpu_bmtree_ext): a
   stream, an event and scratch of its own, made at the first call and
   freed by fd_ed25519_gpu_delete, so tree batches neither share nor size
   the verify path's rings and working sets.

   The device call queues a fixed sequence (fd_bmtree_gpu_launch) whose
   length comes from the shapes alone.  The packed call stages the inputs
   through pinned memory, runs the device call on the slot's stream and
   waits for it within the engine's timeout. */

#include <stdio.h>
#include <string.h>
#include <time.h>
#include <mutex>
#include <vector>
#include "fd_bmtree_gpu_private.h"

#define FD_EXPORT extern "C" __attribute__((visibility("default")))

struct fd_bmtree_ctx {
  fd_ed25519_gpu_t * gpu;
  int           device;
  std::mutex    lock;        /* one packed call at a time: they share the scratch */
  hipStream_t   stream;
  hipEvent_t    done;
  unsigned long d_cap, in_cap, out_cap;
  uint8_t *     d_buf;       /* first | leaves | blob | roots | codes | work */
  uint8_t *     h_in;        /* pinned: first | leaves | blob */
  uint8_t *     h_out;       /* pinned: roots | codes */
  int           busy;        /* a call gave up waiting: `done` has not been seen complete since */
};

static int fd_bmtree_fail( char const * what, hipError_t e ) {
  char buf[256];
  snprintf( buf, sizeof(buf), "%s: %s", what, hipGetErrorString( e ) );
  fd_ed25519_gpu_set_error( buf );
  return FD_ED25519_ERR_GPU;
}

static inline long fd_bmtree_now_ns( void ) {
  struct timespec t; clock_gettime( CLOCK_MONOTONIC, &t );
  return (long)t.tv_sec * 1000000000L + (long)t.tv_nsec;
}

/* the engine's bounded wait: spin for 20 ms, then a query every ~50 us
   until the engine's timeout (< 0: none) */
static int fd_bmtree_wait( fd_bmtree_ctx * c ) {
  long to = fd_ed25519_gpu_timeout( c->gpu ), t0 = fd_bmtree_now_ns();
  for(;;) {
    hipError_t e = hipEventQuery( c->done );
    if( e == hipSuccess ) return 0;
    if( e != hipErrorNotReady ) return fd_bmtree_fail( "hipEventQuery", e );
    long dt = fd_bmtree_now_ns() - t0;
    if( to >= 0 && dt > to ) {
      char buf[128];
      snprintf( buf, sizeof(buf), "bmtree wait: batch not complete after %ld ms", to / 1000000L );
      fd_ed25519_gpu_set_error( buf );
      return FD_ED25519_ERR_GPU;
    }
    if( dt <= 20000000L ) __builtin_ia32_pause();
    else { struct timespec ts = { 0, 50000L }; nanosleep( &ts, NULL ); }
  }
}

static void fd_bmtree_free_scratch( fd_bmtree_ctx * c ) {
  if( c->d_buf ) hipFree( c->d_buf );
  if( c->h_in  ) hipHostFree( c->h_in );
  if( c->h_out ) hipHostFree( c->h_out );
  c->d_buf = c->h_in = c->h_out = NULL; c->d_cap = c->in_cap = c->out_cap = 0UL;
}

/* fd_ed25519_gpu_delete: the engine's own streams have drained.  If ours
   does not within the engine's timeout, the scratch is leaked rather than
   freed under a running kernel. */
static void fd_bmtree_fini( void * p ) {
  fd_bmtree_ctx * c = (fd_bmtree_ctx *)p;
  hipSetDevice( c->device );
  if( hipEventRecord( c->done, c->stream ) != hipSuccess || fd_bmtree_wait( c ) ) return;
  fd_bmtree_free_scratch( c );
  hipEventDestroy( c->done );
  hipStreamDestroy( c->stream );
  delete c;
}

static std::mutex fd_bmtree_make_lock;

static fd_bmtree_ctx * fd_bmtree_ctx_get( fd_ed25519_gpu_t * g ) {
  fd_bmtree_gpu_ext_t * x = fd_ed25519_gpu_bmtree_ext( g );
  std::lock_guard<std::mutex> guard( fd_bmtree_make_lock );
  if( x->ctx ) return (fd_bmtree_ctx *)x->ctx;
  fd_bmtree_ctx * c = new fd_bmtree_ctx();
  c->gpu = g; c->device = fd_ed25519_gpu_device( g );
  hipError_t e = hipSetDevice( c->device );
  if( e == hipSuccess ) e = hipStreamCreateWithFlags( &c->stream, hipStreamNonBlocking );
  if( e == hipSuccess ) {
    e = hipEventCreateWithFlags( &c->done, hipEventDisableTiming );
    if( e != hipSuccess ) hipStreamDestroy( c->stream );
  }
  if( e != hipSuccess ) { fd_bmtree_fail( "bmtree stream", e ); delete c; return NULL; }
  x->ctx = c; x->fini = fd_bmtree_fini;
  return c;
}

static inline unsigned long fd_bmtree_r16( unsigned long n ) { return ( n + 15UL ) & ~15UL; }

/* each buffer grows to what the call needs plus an eighth */
static int fd_bmtree_ensure( fd_bmtree_ctx * c, unsigned long d_sz, unsigned long in_sz, unsigned long out_sz ) {
  hipError_t e = hipSuccess;
  if( d_sz > c->d_cap ) {
    if( c->d_buf ) hipFree( c->d_buf );
    c->d_buf = NULL; c->d_cap = 0UL;
    unsigned long cap = fd_bmtree_r16( d_sz + d_sz/8UL );
    e = hipMalloc( (void **)&c->d_buf, cap );
    if( e == hipSuccess ) c->d_cap = cap;
  }
  if( e == hipSuccess && in_sz > c->in_cap ) {
    if( c->h_in ) hipHostFree( c->h_in );
    c->h_in = NULL; c->in_cap = 0UL;
    unsigned long cap = fd_bmtree_r16( in_sz + in_sz/8UL );
    e = hipHostMalloc( (void **)&c->h_in, cap, hipHostMallocDefault );
    if( e == hipSuccess ) c->in_cap = cap;
  }
  if( e == hipSuccess && out_sz > c->out_cap ) {
    if( c->h_out ) hipHostFree( c->h_out );
    c->h_out = NULL; c->out_cap = 0UL;
    unsigned long cap = fd_bmtree_r16( out_sz + out_sz/8UL );
    e = hipHostMalloc( (void **)&c->h_out, cap, hipHostMallocDefault );
    if( e == hipSuccess ) c->out_cap = cap;
  }
  if( e != hipSuccess ) { fd_bmtree_free_scratch( c ); return fd_bmtree_fail( "bmtree scratch", e ); }
  return 0;
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

/* the plan of a call and its merge lanes: lanes[l] bounds layer l+1 */
static void fd_bmtree_plan_make( fd_bmtree_plan_t * p, unsigned width, unsigned flags, unsigned long n_trees, unsigned long n_leaves,
                                 unsigned long blob_sz, unsigned long leaf_max, uint8_t * d_work, uint32_t lanes[32] ) {
  memset( p, 0, sizeof(*p) );
  p->width = width; p->flags = flags; p->T = (uint32_t)n_trees; p->N = (uint32_t)n_leaves;
  p->leaf_max = (uint32_t)( leaf_max < 0xffffffffUL ? leaf_max : 0xffffffffUL );
  p->blob_sz  = (uint32_t)blob_sz;
  p->L = fd_bmtree_ceil_log2( leaf_max < n_leaves ? leaf_max : n_leaves );
  fd_bmtree_plan_layout( p, d_work );
  for( uint32_t l=0U; l<p->L; l++ ) lanes[l] = (uint32_t)fd_bmtree_layer_bound( n_trees, n_leaves, l + 1U );
}

extern "C" int fd_bmtree_gpu_roots_dev_flags( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                              uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                              void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                              unsigned long root_stride, int * d_codes, void * d_work, void * stream ) {
  if( !fd_bmtree_args_ok( width, flags, FD_BMTREE_GPU_LEAVES_ARE_NODES | FD_BMTREE_GPU_SKIP_EMPTY, n_trees, blob_sz, leaf_max ) ) return FD_ED25519_ERR_ARG;
  if( n_leaves > FD_BMTREE_GPU_LEAVES_MAX ) return FD_ED25519_ERR_ARG;
  if( n_trees && ( !d_first || !d_roots || !d_codes || !d_work ) ) return FD_ED25519_ERR_ARG;
  if( n_leaves && ( !d_leaves || ( blob_sz && !d_blob ) ) ) return FD_ED25519_ERR_ARG;
  if( ( (uintptr_t)d_work & 15UL ) || ( ( (uintptr_t)d_roots | root_stride | (uintptr_t)d_first | (uintptr_t)d_leaves | (uintptr_t)d_codes ) & 3UL ) ||
      ( n_trees && root_stride < 32UL ) ) return FD_ED25519_ERR_ARG;
  if( !n_trees ) return 0;
  if( !gpu ) gpu = fd_ed25519_gpu_default();
  if( !gpu ) return FD_ED25519_ERR_GPU;
  fd_bmtree_ctx * c = fd_bmtree_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_bmtree_fail( "hipSetDevice", e );
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, width, flags, n_trees, n_leaves, blob_sz, leaf_max, (uint8_t *)d_work, lanes );
  p.first = d_first; p.leaves = d_leaves; p.blob = (uint8_t const *)d_blob;
  p.roots = (uint8_t *)d_roots; p.root_stride = root_stride; p.codes = (int32_t *)d_codes;
  e = fd_bmtree_gpu_launch( &p, lanes, stream ? (hipStream_t)stream : c->stream );
  if( e != hipSuccess ) return fd_bmtree_fail( "bmtree launch", e );
  return 0;
}

FD_EXPORT int fd_bmtree_gpu_roots_dev( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                       uint32_t const * d_first, unsigned long n_leaves, fd_bmtree_gpu_leaf_t const * d_leaves,
                                       void const * d_blob, unsigned long blob_sz, unsigned long leaf_max, void * d_roots,
                                       unsigned long root_stride, int * d_codes, void * d_work, void * stream ) {
  if( flags & ~FD_BMTREE_GPU_LEAVES_ARE_NODES ) return FD_ED25519_ERR_ARG;
  return fd_bmtree_gpu_roots_dev_flags( gpu, width, flags, n_trees, d_first, n_leaves, d_leaves, d_blob, blob_sz, leaf_max, d_roots,
                                        root_stride, d_codes, d_work, stream );
}

FD_EXPORT int fd_bmtree_gpu_roots_packed( fd_ed25519_gpu_t * gpu, unsigned width, unsigned flags, unsigned long n_trees,
                                          uint32_t const * leaf_cnt, fd_bmtree_gpu_leaf_t const * leaves, void const * blob,
                                          unsigned long blob_sz, unsigned long leaf_max, void * roots_out, int * codes_out ) {
  if( !fd_bmtree_args_ok( width, flags, FD_BMTREE_GPU_LEAVES_ARE_NODES, n_trees, blob_sz, leaf_max ) ) return FD_ED25519_ERR_ARG;
  if( n_trees && ( !leaf_cnt || !roots_out || !codes_out ) ) return FD_ED25519_ERR_ARG;
  if( !n_trees ) return 0;
  unsigned long n_leaves = 0UL;
  for( unsigned long i=0UL; i<n_trees; i++ ) n_leaves += leaf_cnt[i];
  if( n_leaves > FD_BMTREE_GPU_LEAVES_MAX || ( n_leaves && !leaves ) || ( blob_sz && !blob ) ) return FD_ED25519_ERR_ARG;
  if( !gpu ) gpu = fd_ed25519_gpu_default();
  if( !gpu ) return FD_ED25519_ERR_GPU;
  fd_bmtree_ctx * c = fd_bmtree_ctx_get( gpu );
  if( !c ) return FD_ED25519_ERR_GPU;
  std::lock_guard<std::mutex> guard( c->lock );

  hipError_t e = hipSetDevice( c->device );
  if( e != hipSuccess ) return fd_bmtree_fail( "hipSetDevice", e );
  if( c->busy ) {                       /* an earlier call's launches may still be using the scratch */
    if( fd_bmtree_wait( c ) ) return FD_ED25519_ERR_GPU;
    c->busy = 0;
  }
  unsigned long first_sz = fd_bmtree_r16( 4UL*( n_trees + 1UL ) ), leaf_sz = fd_bmtree_r16( 8UL*n_leaves ), bl_sz = fd_bmtree_r16( blob_sz );
  unsigned long in_sz    = first_sz + leaf_sz + bl_sz;
  unsigned long root_sz  = 32UL*n_trees, code_sz = fd_bmtree_r16( 4UL*n_trees ), out_sz = root_sz + code_sz;
  unsigned long work_sz  = fd_bmtree_gpu_work_sz( n_trees, n_leaves );
  int err = fd_bmtree_ensure( c, in_sz + out_sz + work_sz, in_sz, out_sz );
  if( err ) return err;

  uint32_t * h_first = (uint32_t *)c->h_in;
  unsigned long run = 0UL;
  for( unsigned long i=0UL; i<n_trees; i++ ) { h_first[i] = (uint32_t)run; run += leaf_cnt[i]; }
  h_first[n_trees] = (uint32_t)run;
  if( n_leaves ) memcpy( c->h_in + first_sz, leaves, 8UL*n_leaves );
  if( blob_sz  ) memcpy( c->h_in + first_sz + leaf_sz, blob, blob_sz );

  uint8_t * d_in = c->d_buf, * d_out = d_in + in_sz, * d_work = d_out + out_sz;
  fd_bmtree_plan_t p; uint32_t lanes[32];
  fd_bmtree_plan_make( &p, width, flags, n_trees, n_leaves, blob_sz, leaf_max, d_work, lanes );
  p.first = (uint32_t const *)d_in; p.leaves = (fd_bmtree_gpu_leaf_t const *)( d_in + first_sz ); p.blob = d_in + first_sz + leaf_sz;
  p.roots = d_out; p.root_stride = 32UL; p.codes = (int32_t *)( d_out + root_sz );
  /* the host knows the counts: the lanes of the trees the count rules keep */
  for( uint32_t l=0U; l<p.L; l++ ) lanes[l] = 0U;
  for( unsigned long i=0UL; i<n_trees; i++ ) {
    unsigned long cc = leaf_cnt[i] <= leaf_max ? leaf_cnt[i] : 0UL;
    for( uint32_t l=0U; l<p.L && cc>1UL; l++ ) { cc = ( cc + 1UL ) >> 1; lanes[l] += (uint32_t)cc; }
  }

  e = hipMemcpyAsync( d_in, c->h_in, in_sz, hipMemcpyHostToDevice, c->stream );
  if( e == hipSuccess ) e = fd_bmtree_gpu_launch( &p, lanes, c->stream );
  if( e == hipSuccess ) e = hipMemcpyAsync( c->h_out, d_out, out_sz, hipMemcpyDeviceToHost, c->stream );
  /* whatever was queued is waited for, also after a failed enqueue */
  hipError_t e2 = hipEventRecord( c->done, c->stream );
  if( e2 != hipSuccess ) { c->busy = 1; return fd_bmtree_fail( "hipEventRecord", e2 ); }
  if( fd_bmtree_wait( c ) ) { c->busy = 1; return FD_ED25519_ERR_GPU; }
  if( e != hipSuccess ) return fd_bmtree_fail( "bmtree launch", e );

  memcpy( roots_out, c->h_out, root_sz );
  memcpy( codes_out, c->h_out + root_sz, 4UL*n_trees );
  return 0;
}
