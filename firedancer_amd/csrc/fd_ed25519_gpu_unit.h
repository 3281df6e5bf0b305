#ifndef HEADER_fd_ed25519_gpu_unit_h
#define HEADER_fd_ed25519_gpu_unit_h

/* fd_ed25519_gpu_unit.h -- the engine's side units (fd_poh_gpu.cpp,
   fd_bmtree_gpu.cpp): host code that hangs off an engine through a slot,
   with a stream, a completion event and scratch of its own, made at the
   first call and torn down by fd_ed25519_gpu_delete, so its batches neither
   share nor size the verify path's rings and working sets.  Private to the
   library: everything here is hidden from the dynamic table. */

#include <mutex>
#include <hip/hip_runtime.h>
#include "fd_ed25519_gpu.h"

#define FD_HIDDEN extern "C" __attribute__((visibility("hidden")))

enum { FD_GPU_UNIT_POH, FD_GPU_UNIT_BMTREE, FD_GPU_UNIT_CNT };   /* the engine's slots, in teardown order */

#define FD_GPU_UNIT_BUF_MAX 5

/* An owner derives its state from this and adds what is its own. */
struct __attribute__((visibility("hidden"))) fd_gpu_unit {
  char const *       name;   /* leads the unit's error texts: "poh", "bmtree" */
  fd_ed25519_gpu_t * gpu;
  int                device;
  std::mutex         lock;   /* one packed call at a time: they share the scratch */
  hipStream_t        stream;
  hipEvent_t         done;
  int                busy;   /* a call gave up waiting: `done` has not been seen complete since */
  struct { uint8_t * p; unsigned long cap; int pinned; } buf[FD_GPU_UNIT_BUF_MAX];   /* scratch: device or pinned host memory */
  virtual ~fd_gpu_unit() {}
};

/* in fd_ed25519_gpu_host.cpp: the engine's slots, and its bounded wait (the
   library's one poll loop) on ev within the engine's timeout: 0, or
   FD_ED25519_ERR_GPU with "<who> wait: batch not complete after .. ms" */
FD_HIDDEN fd_gpu_unit ** fd_ed25519_gpu_units( fd_ed25519_gpu_t * gpu );
FD_HIDDEN int fd_ed25519_gpu_unit_wait( fd_ed25519_gpu_t * gpu, hipEvent_t ev, char const * who );

/* "what: <HIP's text>" into the thread's last error; FD_ED25519_ERR_GPU */
FD_HIDDEN int fd_gpu_unit_fail( char const * what, hipError_t e );

/* The unit in slot idx of gpu (NULL: the default engine), made by make on
   first use.  NULL, with the last error set, when there is no engine or the
   stream or the event cannot be made: the caller's FD_ED25519_ERR_GPU. */
FD_HIDDEN fd_gpu_unit * fd_gpu_unit_get_raw( fd_ed25519_gpu_t * gpu, int idx, char const * name, fd_gpu_unit * (*make)( void ) );
template<class T> static inline T * fd_gpu_unit_get( fd_ed25519_gpu_t * gpu, int idx, char const * name ) {
  return static_cast<T *>( fd_gpu_unit_get_raw( gpu, idx, name, []() -> fd_gpu_unit * { return new T(); } ) );
}

/* A packed call, under u->lock: begin (the device is made current, and an
   earlier call that gave up waiting is waited out, for its launches may
   still be using the scratch), grow what the call needs, enqueue on
   u->stream, finish with the enqueue's result.  finish waits for whatever
   was queued, also after a failed enqueue, marks the unit busy when the
   record or the wait fails, and only then reports "<name> launch". */
FD_HIDDEN int fd_gpu_unit_begin( fd_gpu_unit * u );
FD_HIDDEN int fd_gpu_unit_finish( fd_gpu_unit * u, hipError_t enqueued );

/* buf[i] holds at least need bytes: device memory, or pinned host memory.
   A buffer that is too small is replaced by one of need plus an eighth,
   rounded up to 16.  When the allocation fails all of the unit's scratch
   is released and the call fails with "<name> scratch". */
FD_HIDDEN int fd_gpu_unit_grow( fd_gpu_unit * u, int i, int pinned, unsigned long need );

/* fd_ed25519_gpu_delete, once the engine's own streams have drained.  If
   the unit's does not within the engine's timeout, the unit is leaked
   rather than freed under a running kernel. */
FD_HIDDEN void fd_gpu_unit_fini( fd_gpu_unit * u );

static inline unsigned long fd_gpu_r16( unsigned long n ) { return ( n + 15UL ) & ~15UL; }

#endif /* HEADER_fd_ed25519_gpu_unit_h */
