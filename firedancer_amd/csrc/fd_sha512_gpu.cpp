/* fd_sha512_gpu.cpp -- ballet SHA-512 batch API on the GPU engine
   (include/fd_sha512_gpu.h; reference contract
   src/ballet/sha512/fd_sha512.h:223-294).  fini packs the queued
   messages into engine-sized chunks (pinned staging buffers lent by the
   engine, so each message is copied once), hashes each chunk on the
   device and scatters the digests to the callers' hash pointers.  A
   message no chunk can hold (larger than the engine's blob, or than a
   32-bit descriptor) goes through the long runner instead
   (fd_sha512_gpu_long, fd_ed25519_gpu_host.cpp), so no size is refused. */

#include <string.h>
#include <vector>
#include "fd_sha512_gpu.h"
#include "fd_sha512_gpu_private.h"

#define FD_EXPORT extern "C" __attribute__((visibility("default")))

struct fd_sha512_gpu_item { uint8_t const * data; unsigned long sz; void * hash; };

struct fd_sha512_gpu_batch {
  fd_ed25519_gpu_t *              gpu;
  int                             is384;
  std::vector<fd_sha512_gpu_item> q;
  std::vector<uint8_t>            dig;
};

FD_EXPORT fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_new( fd_ed25519_gpu_t * gpu, int is384 ) {
  if( !gpu ) gpu = fd_ed25519_gpu_default();
  if( !gpu ) return NULL;
  fd_sha512_gpu_batch_t * b = new fd_sha512_gpu_batch_t();
  b->gpu = gpu; b->is384 = !!is384;
  return b;
}

FD_EXPORT void fd_sha512_gpu_batch_delete( fd_sha512_gpu_batch_t * b ) { delete b; }

FD_EXPORT fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_init( fd_sha512_gpu_batch_t * b ) {
  b->q.clear();
  return b;
}

FD_EXPORT fd_sha512_gpu_batch_t * fd_sha512_gpu_batch_add( fd_sha512_gpu_batch_t * b, void const * data,
                                                          unsigned long sz, void * hash ) {
  fd_sha512_gpu_item it = { (uint8_t const *)data, sz, hash };
  b->q.push_back( it );
  return b;
}

FD_EXPORT void * fd_sha512_gpu_batch_abort( fd_sha512_gpu_batch_t * b ) {
  b->q.clear();
  return (void *)b;
}


/* a message the packed path cannot take: larger than the staging blob or
   than a 32-bit descriptor */
static inline int fd_sha_is_long( unsigned long sz, unsigned long max_blob ) { return sz > max_blob || sz > 0xffffffffUL; }

/* n messages that all fit the packed path, in engine-sized chunks */
static int fd_sha_run_short( fd_ed25519_gpu_t * g, fd_sha512_gpu_item const * q, size_t n, int is384, std::vector<uint8_t> & dig ) {
  unsigned long max_sigs = fd_ed25519_gpu_max_sigs( g ), max_blob = fd_ed25519_gpu_max_blob( g );
  unsigned long hsz = is384 ? 48UL : 64UL;
  dig.resize( max_sigs * hsz );
  size_t i = 0;
  while( i < n ) {
    void * blob; fd_ed25519_gpu_desc_t * desc;
    if( fd_ed25519_gpu_stage( g, &blob, &desc ) ) return FD_ED25519_ERR_GPU;
    uint8_t * bl = (uint8_t *)blob;
    unsigned long used = 0, cnt = 0;
    while( i + cnt < n && cnt < max_sigs && used + q[i+cnt].sz <= max_blob ) {
      fd_sha512_gpu_item const & it = q[i+cnt];
      if( it.sz ) memcpy( bl + used, it.data, it.sz );
      desc[cnt].sig_off = 0; desc[cnt].pub_off = 0;
      desc[cnt].msg_off = (uint32_t)used; desc[cnt].msg_sz = (uint32_t)it.sz;
      used = (used + it.sz + 7UL) & ~7UL;
      if( used > max_blob ) used = max_blob;
      cnt++;
    }
    int err = fd_ed25519_gpu_sha512_packed( g, cnt, blob, used, desc, dig.data(), is384 );
    if( err ) { fd_ed25519_gpu_unstage( g, blob ); return err; }
    for( unsigned long k=0; k<cnt; k++ ) memcpy( q[i+k].hash, dig.data() + k*hsz, hsz );
    i += cnt;
  }
  return 0;
}

/* Every queued message: those that fit the packed path exactly as a queue
   without long messages runs them (the same engine calls in the same
   order), the long ones after, through the long runner. */
static int fd_sha_run( fd_ed25519_gpu_t * g, std::vector<fd_sha512_gpu_item> const & q, int is384, std::vector<uint8_t> & dig ) {
  unsigned long max_blob = fd_ed25519_gpu_max_blob( g );
  size_t n = q.size(), nl = 0;
  for( size_t i=0; i<n; i++ ) nl += (size_t)fd_sha_is_long( q[i].sz, max_blob );
  if( !nl ) return fd_sha_run_short( g, q.data(), n, is384, dig );
  std::vector<fd_sha512_gpu_item> sq; sq.reserve( n - nl );
  std::vector<fd_sha_long_req_t>  lq; lq.reserve( nl );
  for( size_t i=0; i<n; i++ ) {
    if( fd_sha_is_long( q[i].sz, max_blob ) ) lq.push_back( { q[i].data, q[i].sz, q[i].hash } );
    else                                      sq.push_back( q[i] );
  }
  int err = sq.empty() ? 0 : fd_sha_run_short( g, sq.data(), sq.size(), is384, dig );
  if( err ) return err;
  return fd_sha512_gpu_long( g, lq.size(), lq.data(), is384 );
}

FD_EXPORT void * fd_sha512_gpu_batch_fini( fd_sha512_gpu_batch_t * b ) {
  int err = fd_sha_run( b->gpu, b->q, b->is384, b->dig );
  b->q.clear();
  return err ? NULL : (void *)b;
}

FD_EXPORT int fd_ed25519_gpu_sha512_ptrs( fd_ed25519_gpu_t * gpu, unsigned long n, void const * const * data, unsigned long const * sz,
                                          void * hash_out, int is384 ) {
  if( !gpu ) gpu = fd_ed25519_gpu_default();
  if( !gpu ) return FD_ED25519_ERR_GPU;
  if( n && ( !data || !sz || !hash_out ) ) return FD_ED25519_ERR_ARG;
  unsigned long hsz = is384 ? 48UL : 64UL;
  for( unsigned long i=0; i<n; i++ ) if( sz[i] && !data[i] ) return FD_ED25519_ERR_ARG;
  std::vector<fd_sha512_gpu_item> q( n );
  for( unsigned long i=0; i<n; i++ ) q[i] = { (uint8_t const *)data[i], sz[i], (uint8_t *)hash_out + i*hsz };
  std::vector<uint8_t> dig;
  return fd_sha_run( gpu, q, !!is384, dig );
}
