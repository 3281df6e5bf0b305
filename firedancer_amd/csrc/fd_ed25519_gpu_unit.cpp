/* fd_ed25519_gpu_unit.cpp -- what the engine's side units have in common
   (fd_ed25519_gpu_unit.h): creation on first use, the packed call's
   begin / grow / finish, and teardown. */

#include <stdio.h>
#include "fd_ed25519_gpu_unit.h"

extern "C" void fd_ed25519_gpu_set_error( char const * what );   /* fd_ed25519_gpu_host.cpp: this thread's last error */

int fd_gpu_unit_fail( char const * what, hipError_t e ) {
  char buf[256];
  snprintf( buf, sizeof(buf), "%s: %s", what, hipGetErrorString( e ) );
  fd_ed25519_gpu_set_error( buf );
  return FD_ED25519_ERR_GPU;
}

/* "<name> <what>: <HIP's text>" */
static int fd_gpu_unit_fail_as( fd_gpu_unit const * u, char const * what, hipError_t e ) {
  char buf[64];
  snprintf( buf, sizeof(buf), "%s %s", u->name, what );
  return fd_gpu_unit_fail( buf, e );
}

static std::mutex fd_gpu_unit_make_lock;

fd_gpu_unit * fd_gpu_unit_get_raw( fd_ed25519_gpu_t * gpu, int idx, char const * name, fd_gpu_unit * (*make)( void ) ) {
  if( !gpu ) gpu = fd_ed25519_gpu_default();
  if( !gpu ) return NULL;
  fd_gpu_unit ** slot = fd_ed25519_gpu_units( gpu ) + idx;
  std::lock_guard<std::mutex> guard( fd_gpu_unit_make_lock );
  if( *slot ) return *slot;
  fd_gpu_unit * u = make();
  u->name = name; u->gpu = gpu; u->device = fd_ed25519_gpu_device( gpu );
  hipError_t e = hipSetDevice( u->device );
  if( e == hipSuccess ) e = hipStreamCreateWithFlags( &u->stream, hipStreamNonBlocking );
  if( e == hipSuccess ) {
    e = hipEventCreateWithFlags( &u->done, hipEventDisableTiming );
    if( e != hipSuccess ) hipStreamDestroy( u->stream );
  }
  if( e != hipSuccess ) { fd_gpu_unit_fail_as( u, "stream", e ); delete u; return NULL; }
  return *slot = u;
}

int fd_gpu_unit_begin( fd_gpu_unit * u ) {
  hipError_t e = hipSetDevice( u->device );
  if( e != hipSuccess ) return fd_gpu_unit_fail( "hipSetDevice", e );
  if( u->busy ) {
    if( fd_ed25519_gpu_unit_wait( u->gpu, u->done, u->name ) ) return FD_ED25519_ERR_GPU;
    u->busy = 0;
  }
  return 0;
}

int fd_gpu_unit_finish( fd_gpu_unit * u, hipError_t enqueued ) {
  hipError_t e = hipEventRecord( u->done, u->stream );
  if( e != hipSuccess ) { u->busy = 1; return fd_gpu_unit_fail( "hipEventRecord", e ); }
  if( fd_ed25519_gpu_unit_wait( u->gpu, u->done, u->name ) ) { u->busy = 1; return FD_ED25519_ERR_GPU; }
  if( enqueued != hipSuccess ) return fd_gpu_unit_fail_as( u, "launch", enqueued );
  return 0;
}

static void fd_gpu_unit_free( fd_gpu_unit * u, int i ) {
  if( u->buf[i].p ) { if( u->buf[i].pinned ) hipHostFree( u->buf[i].p ); else hipFree( u->buf[i].p ); }
  u->buf[i].p = NULL; u->buf[i].cap = 0UL;
}

static void fd_gpu_unit_free_scratch( fd_gpu_unit * u ) {
  for( int i=0; i<FD_GPU_UNIT_BUF_MAX; i++ ) fd_gpu_unit_free( u, i );
}

int fd_gpu_unit_grow( fd_gpu_unit * u, int i, int pinned, unsigned long need ) {
  if( need <= u->buf[i].cap ) return 0;
  fd_gpu_unit_free( u, i );
  unsigned long cap = fd_gpu_r16( need + need/8UL );
  hipError_t e = pinned ? hipHostMalloc( (void **)&u->buf[i].p, cap, hipHostMallocDefault ) : hipMalloc( (void **)&u->buf[i].p, cap );
  if( e != hipSuccess ) { u->buf[i].p = NULL; fd_gpu_unit_free_scratch( u ); return fd_gpu_unit_fail_as( u, "scratch", e ); }
  u->buf[i].cap = cap; u->buf[i].pinned = pinned;
  return 0;
}

void fd_gpu_unit_fini( fd_gpu_unit * u ) {
  if( !u ) return;
  hipSetDevice( u->device );
  if( hipEventRecord( u->done, u->stream ) != hipSuccess || fd_ed25519_gpu_unit_wait( u->gpu, u->done, u->name ) ) return;
  fd_gpu_unit_free_scratch( u );
  hipEventDestroy( u->done );
  hipStreamDestroy( u->stream );
  delete u;
}
