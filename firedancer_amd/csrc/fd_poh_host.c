/* fd_poh_host.c -- Proof-of-History on the host (include/fd_poh_gpu.h):
   the reference's fd_poh_append and fd_poh_mixin
   (src/ballet/poh/fd_poh.c:3-24) built from the two specialised SHA-256
   bodies the device kernel uses (fd_poh_core.h), the entry semantics on
   host threads (fd_poh_verify_batch: the bench's yardstick and the CPU
   tests' subject), and fd_poh_gpu_chain.  No device code. */

#include <string.h>
#include <pthread.h>
#include "fd_poh_gpu.h"
#include "fd_poh_core.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT fd_poh_state_t * fd_poh_append( fd_poh_state_t * poh, unsigned long n ) {
  uint8_t * p = (uint8_t *)poh;
  uint32_t s[8];
  fd_poh_load( s, p );
  while( n-- ) fd_poh_step( s );
  fd_poh_store( p, s );
  return poh;
}

EXPORT fd_poh_state_t * fd_poh_mixin( fd_poh_state_t * poh, uint8_t const * mixin ) {
  uint8_t * p = (uint8_t *)poh;
  uint32_t s[8], m[8];
  fd_poh_load( s, p );
  fd_poh_load( m, mixin );
  fd_poh_mix( s, m );
  fd_poh_store( p, s );
  return poh;
}

/* one entry: its code, and its final state to st32 (zeros where it is refused) */
static int fd_poh_entry_run( fd_poh_gpu_entry_t const * e, unsigned long n_max, uint8_t * st32 ) {
  if( ( e->flags & ~FD_POH_GPU_MIXIN ) || e->_pad || e->n > n_max ) {
    memset( st32, 0, 32 );
    return FD_ED25519_ERR_ARG;
  }
  uint32_t s[8], m[8];
  fd_poh_load( s, e->start );
  for( uint64_t k=e->n; k; k-- ) fd_poh_step( s );
  if( e->flags & FD_POH_GPU_MIXIN ) { fd_poh_load( m, e->mixin ); fd_poh_mix( s, m ); }
  fd_poh_store( st32, s );
  return memcmp( st32, e->expect, 32 ) ? FD_POH_ERR_HASH : 0;
}

/* entries are taken in runs of this many from a shared cursor */
#define FD_POH_DEAL 8UL

typedef struct {
  unsigned long              n;
  fd_poh_gpu_entry_t const * ent;
  unsigned long              n_max;
  int *                      out;
  uint8_t *                  st;
  unsigned long *            next;
} fd_poh_job_t;

static void * fd_poh_worker( void * arg ) {
  fd_poh_job_t * j = (fd_poh_job_t *)arg;
  for(;;) {
    unsigned long i0 = __atomic_fetch_add( j->next, FD_POH_DEAL, __ATOMIC_RELAXED );
    if( i0 >= j->n ) break;
    unsigned long i1 = i0 + FD_POH_DEAL < j->n ? i0 + FD_POH_DEAL : j->n;
    for( unsigned long i=i0; i<i1; i++ ) {
      uint8_t tmp[32];
      j->out[i] = fd_poh_entry_run( j->ent + i, j->n_max, j->st ? j->st + 32UL*i : tmp );
    }
  }
  return NULL;
}

EXPORT int fd_poh_verify_batch( unsigned long n, fd_poh_gpu_entry_t const * entries, unsigned long n_max, int * out,
                                void * state_out_opt, int nthreads ) {
  if( nthreads < 1 || nthreads > 256 ) return FD_ED25519_ERR_ARG;
  if( n && ( !entries || !out ) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  unsigned long next = 0UL;
  fd_poh_job_t job = { n, entries, n_max, out, (uint8_t *)state_out_opt, &next };
  unsigned long runs = ( n + FD_POH_DEAL - 1UL ) / FD_POH_DEAL;
  if( (unsigned long)nthreads > runs ) nthreads = (int)runs;
  pthread_t th[256];
  int started = 0;
  for( int t=1; t<nthreads; t++ ) {
    if( pthread_create( &th[started], NULL, fd_poh_worker, &job ) ) break;   /* fewer threads: the others take its share */
    started++;
  }
  fd_poh_worker( &job );
  for( int t=0; t<started; t++ ) pthread_join( th[t], NULL );
  return 0;
}

EXPORT void fd_poh_gpu_chain( unsigned long n, uint8_t const * seed, uint8_t const * hashes, fd_poh_gpu_entry_t * entries ) {
  for( unsigned long i=0; i<n; i++ ) {
    memcpy( entries[i].start,  i ? hashes + 32UL*(i-1UL) : seed, 32 );
    memcpy( entries[i].expect, hashes + 32UL*i, 32 );
  }
}
