/* fd_ed25519_gpu_host.cpp -- host runtime of the MI355X Ed25519 engine
   (the util/gpu shim of SURVEY.md section 7, step 2).

   One engine per device.  The engine owns:
     - device buffers for one batch of capacity (max_sigs, max_blob) per
       ring slot: blob, descriptors, result codes and the HBM working set;
     - depth (default 3, up to 8) pinned host slots (blob, desc, out) and one HIP stream
       per slot, so batch b+1's H2D copy overlaps batch b's kernels and
       batch b-1's D2H copy (double/triple buffering);
   All allocation happens in fd_ed25519_gpu_new (the verify tile calls it
   from init(), before the sandbox closes the syscalls HIP needs,
   src/app/frank/fd_frank_verify.c:7-20).

   Nothing here verifies on the CPU: every code comes from the device. */

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <mutex>
#include <deque>
#include <condition_variable>
#include <vector>
#include <atomic>
#include <map>
#include "fd_ed25519_gpu_private.h"
#include "fd_ed25519_gpu_diag.h"
#include "fd_ed25519_gpu_sign_private.h"
#include "fd_ed25519_gpu_txn_private.h"
#include "fd_ed25519_gpu_txn_claim.h"
#include "fd_sha512_gpu_private.h"
#include "fd_ed25519_gpu_unit.h"

#define FD_GPU_DEPTH_DEFAULT 3
#define FD_GPU_DEPTH_MAX     8
#ifndef FD_CU_GROUPS
#define FD_CU_GROUPS         4   /* max default CU groups for small ring batches (1: none) */
#endif
#define FD_REG_MAX           16  /* registered host regions per engine */
#define FD_DEV_STATS_MAX     64  /* pipelined launches timed per stats window */
#define FD_BLOB_PAD  64UL

static thread_local char fd_gpu_err[256];

static int fd_gpu_fail( char const * what, hipError_t e ) {
  snprintf( fd_gpu_err, sizeof(fd_gpu_err), "%s: %s", what, hipGetErrorString( e ) );
  return FD_ED25519_ERR_GPU;
}
static void fd_gpu_fail_q( char const * what, hipError_t e ) { (void)fd_gpu_fail( what, e ); }

/* blocking polls spin this long before they start sleeping between queries */
#define FD_POLL_SPIN_NS 20000000L
/* default bound on one blocking wait (fd_ed25519_gpu_set_timeout): a
   4096-signature batch takes ~0.8 ms and a 1M-signature launch ~17 ms, so
   10 s only fires on a wedged queue (the reference's accelerator poll is
   bounded the same way, src/wiredancer/c/wd_f1.h:25 WD_TRY_LIMIT) */
#define FD_WAIT_TIMEOUT_NS_DEFAULT 10000000000L

static inline long fd_now_ns( void ) {
  struct timespec t; clock_gettime( CLOCK_MONOTONIC, &t );
  return (long)t.tv_sec * 1000000000L + (long)t.tv_nsec;
}

/* The engine's ring lock.  Its callers are tiles, each spinning on a core
   of its own, and on an engine shared by tiles (fd_verify_tile_args_t.
   shared_gpu) two of them poll and submit through it every few
   microseconds.  std::mutex parks a contended caller in the kernel at
   once, and on a host with other work the woken thread can wait out
   another task's time slice (milliseconds) before it runs again: spin on
   try_lock for a while first (holders keep it for one HIP enqueue or
   query, microseconds), then block. */
struct fd_ring_lock {
  std::mutex m;
  void lock( void ) {
    if( m.try_lock() ) return;
    long const t0 = fd_now_ns();
    do {
      for( int i=0; i<16; i++ ) __builtin_ia32_pause();
      if( m.try_lock() ) return;
    } while( fd_now_ns() - t0 < 200000L );
    m.lock();
  }
  bool try_lock( void ) { return m.try_lock(); }
  void unlock( void ) { m.unlock(); }
};

/* Bounded wait on a completion query: spin (as a tile busy-polls its
   rings; a sleeping wake-up adds tens of microseconds to a ~0.8 ms batch
   round trip) for up to spin_ns, then query every ~50 us until timeout_ns
   (< 0: no bound).  query returns 1 ready, 0 not yet, < 0 failed.  Returns
   1 ready, 0 timed out, < 0 the query's failure. */
static int fd_wait_query( int (*query)( void * ), void * ctx, long spin_ns, long timeout_ns ) {
  int r = query( ctx );
  if( r ) return r;
  long t0 = fd_now_ns();
  for(;;) {
    long dt = fd_now_ns() - t0;
    if( timeout_ns >= 0 && dt > timeout_ns ) return 0;
    if( dt <= spin_ns ) __builtin_ia32_pause();
    else { struct timespec ts = { 0, 50000L }; nanosleep( &ts, NULL ); }
    if( (r = query( ctx )) ) return r;
  }
}

static int fd_event_query( void * ev ) {
  hipError_t e = hipEventQuery( (hipEvent_t)ev );
  if( e == hipSuccess ) return 1;
  if( e == hipErrorNotReady ) return 0;
  fd_gpu_fail_q( "hipEventQuery", e );
  return -1;
}

/* a blocking wait on a batch's completion: what query returned (> 0), or
   FD_ED25519_ERR_GPU on a runtime failure or after timeout_ns (the batch
   may still complete; the caller may poll again).  who: names a side unit
   in the text, or "" */
static int fd_batch_wait( int (*query)( void * ), void * ctx, long timeout_ns, char const * who ) {
  int r = fd_wait_query( query, ctx, FD_POLL_SPIN_NS, timeout_ns );
  if( r == 0 ) snprintf( fd_gpu_err, sizeof(fd_gpu_err), "%s%swait: batch not complete after %ld ms", who, *who ? " " : "", timeout_ns / 1000000L );
  return r > 0 ? r : FD_ED25519_ERR_GPU;
}

/* wait for a slot's completion event: 0 done, else FD_ED25519_ERR_GPU */
static int fd_event_wait( hipEvent_t ev, long timeout_ns ) {
  return fd_batch_wait( fd_event_query, (void *)ev, timeout_ns, "" ) > 0 ? 0 : FD_ED25519_ERR_GPU;
}

/* fd_event_wait for the side units, within the engine's timeout */
int fd_ed25519_gpu_unit_wait( fd_ed25519_gpu_t * g, hipEvent_t ev, char const * who ) {
  return fd_batch_wait( fd_event_query, (void *)ev, fd_ed25519_gpu_timeout( g ), who ) > 0 ? 0 : FD_ED25519_ERR_GPU;
}

/* Self-test of the bounded wait without a device (tests/test_abi.py): a
   fake completion that becomes ready ready_after_ns after the call (< 0:
   never, a stuck batch).  Returns 1 ready, 0 timed out. */
struct fd_fake_ticket { long ready_at; };
static int fd_fake_query( void * ctx ) {
  fd_fake_ticket * f = (fd_fake_ticket *)ctx;
  return f->ready_at >= 0 && fd_now_ns() >= f->ready_at;
}
extern "C" int fd_ed25519_gpu_wait_selftest( long timeout_ns, long ready_after_ns ) {
  fd_fake_ticket f = { ready_after_ns < 0 ? -1L : fd_now_ns() + ready_after_ns };
  return fd_wait_query( fd_fake_query, &f, 1000000L, timeout_ns );
}

/* direct-output batches of at most this many signatures can be collected
   by a blocking poll as soon as every code has landed in pinned memory,
   before the batch's completion event fires (fd_codes_query) */
#define FD_EARLY_MAX_DEFAULT 64UL
/* what h_out holds until the DSM writes a code there (no code is this) */
#define FD_CODE_PENDING ((int32_t)0x7eadc0de)

static inline unsigned long fd_desc_off( unsigned long blob_sz ) { return (blob_sz + FD_BLOB_PAD + 15UL) & ~15UL; }
extern "C" unsigned long fd_ed25519_gpu_desc_offset( unsigned long blob_sz ) { return fd_desc_off( blob_sz ); }

struct fd_ed25519_gpu_slot {
  /* pinned host staging */
  uint8_t *               h_blob;
  fd_ed25519_gpu_desc_t * h_desc;
  fd_ed25519_gpu_desc_t * h_desc_dev;   /* h_desc as the device addresses it (mapped), or NULL */
  int32_t *               h_out;
  int32_t *               h_out_dev;  /* h_out as the device addresses it (coherent, mapped), or NULL */
  /* device */
  uint8_t *               d_blob;
  fd_ed25519_gpu_desc_t * d_desc;
  int32_t *               d_out;
  fd_ed25519_gpu_work_t   work;
  void *                  d_work_base;
  hipStream_t             stream;
  hipStream_t             mstream;  /* the slot's CU group (small batches on a ring of depth > 1), or NULL */
  hipEvent_t              done;
  unsigned long           n;
  unsigned long           ticket;   /* 0 = free */
  int                     staged;   /* pinned buffers lent out by fd_ed25519_gpu_stage */
  int                     orphan;   /* a synchronous call timed out on it: reclaimed once its event completes */
  int                     early;    /* codes go straight to h_out over a sentinel: a blocking poll may take them as they land */
  int                     retiring; /* its codes were taken early: reclaimed once its event completes */
  uint8_t *               h_dig;    /* pinned digests (SHA-512 batch), allocated on first use */
  uint8_t *               h_sgn;    /* pinned signing results (100 B per signature), allocated on first use */
  hipEvent_t              sha_ev[2]; /* long plain hashes: the kernel that read half h of the blob has finished (first use) */
  /* transaction batches on the ring (fd_ed25519_gpu_submit_txns): the
     slot's own scratch, allocated by fd_txn_ring_ensure */
  unsigned long                 n_txn;     /* transactions of the batch in flight; 0: a descriptor batch */
  fd_ed25519_gpu_desc_t *       t_desc;    /* device: max_sigs descriptors, written by fd_k_txn_ring_front */
  fd_ed25519_gpu_txn_result_t * t_res;     /* device: max_sigs results, between front and reduce */
  fd_ed25519_gpu_txn_result_t * h_res;     /* pinned, mapped, coherent: the final results */
  fd_ed25519_gpu_txn_result_t * h_res_dev; /* h_res as the device addresses it */
};

/* one of the two scratch sets of the transaction calls (fd_ed25519_gpu_txn.h) */
struct fd_txn_set {
  fd_txn_meta_t *         meta;    /* txn_cap entries */
  uint32_t *              part;    /* fd_txn_part_cnt( txn_cap ) words */
  fd_ed25519_gpu_desc_t * desc;    /* max_sigs slots */
  int32_t *               codes;   /* max_sigs codes */
  hipEvent_t              done;    /* the last call that used the set has finished with it */
};

struct fd_ed25519_gpu {
  int           device;
  unsigned long max_sigs;
  unsigned long max_blob;
  unsigned long next_ticket;
  int           depth;
  int           mode;     /* FD_ED25519_GPU_MODE_* */
  unsigned long pool_min; /* batches >= this take the pooled DSM */
  unsigned long quad_max; /* smaller batches <= this take the quad-lane DSM */
  unsigned long oct_max;  /* and batches <= this the eight-lane DSM */
  unsigned long out_direct_max;  /* ring batches <= this get their codes written to pinned memory by the DSM */
  unsigned long early_max;       /* and batches <= this may be collected before their completion event (fd_codes_query) */
  unsigned long blob_cap;        /* bytes of a slot's blob buffers (padded blob + descriptors) */
  unsigned long mask_max; /* ring batches <= this run on their slot's CU group */
  int           groups;   /* CU groups the ring's slots are spread over (1: none) */
  int           group_always; /* experiments (FD_ED25519_GPU_GROUP_ALWAYS=1): a lone ring batch also runs on its CU group */
  int           ncu;
  struct { uint8_t const * p; unsigned long sz; } reg[FD_REG_MAX];   /* hipHostRegister'ed source regions */
  long          timeout_ns; /* bound on one blocking wait (< 0: none); atomic: set from any thread, read by waiters and feeders */
  fd_ed25519_gpu_slot slot[FD_GPU_DEPTH_MAX];
  /* device-resident path (verify_dev / _timed): its own HBM working sets,
     so it never shares scratch with a ring batch */
  /* two working sets, used alternately by successive device-resident
     launches: launch k's front end (prep, decomp, Ai tables) runs on
     dev_sf while launch k-1's DSM runs on dev_sb, so it fills the SIMDs
     the DSM's last round of waves leaves idle (fd_dev_launch) */
  fd_ed25519_gpu_work_t dev_work[2];
  void *        d_dev_work_base[2];
  hipStream_t   dev_sf, dev_sb;
  hipEvent_t    dev_in[2], dev_front[2], dev_back[2];   /* dev_back[b]: working set b free */
  unsigned long dev_seq;
  std::mutex    dev_lock;
  /* per-kernel HIP events of pipelined launches (fd_ed25519_gpu_dev_stats_*) */
  int           dev_stats_on;
  unsigned long dev_stats_cnt;
  hipEvent_t    dev_ev[FD_DEV_STATS_MAX][FD_EV_CNT];
  hipEvent_t    kev[FD_EV_CNT];   /* per-kernel timing events */
  /* whole transactions (fd_ed25519_gpu_txns_reserve; under dev_lock):
     successive calls alternate between two scratch sets; the packed call
     stages entries, results, codes and descriptors in txn_pk */
  fd_txn_set    txn_set[2];
  unsigned long txn_cap;          /* transactions the sets and the staging take */
  unsigned long txn_seq;
  uint8_t *     d_txn_pk;
  uint8_t *     h_txn_pk;         /* pinned, the same layout */
  unsigned long txn_pk_sz;
  hipEvent_t    txn_ev[6];        /* per-kernel timing events of the transaction kernels */
  /* transaction batches on the ring (under the ring lock) */
  unsigned long txn_ring_allocs;  /* slots whose transaction scratch was allocated (fd_ed25519_gpu_txn_ring_allocs) */
  hipEvent_t    txn_ring_ev[4];   /* fd_ed25519_gpu_txn_ring_timed: around the front kernel and the reduce */
  fd_gpu_unit * unit[FD_GPU_UNIT_CNT];   /* side units (fd_ed25519_gpu_unit.h): Proof-of-History chains, Merkle trees; made on first use */
  fd_ring_lock  lock;
};

fd_gpu_unit ** fd_ed25519_gpu_units( fd_ed25519_gpu_t * g ) { return g->unit; }

static inline long fd_timeout( fd_ed25519_gpu_t const * g ) { return __atomic_load_n( &g->timeout_ns, __ATOMIC_RELAXED ); }

#define HIPCHK(call) do { hipError_t e_ = (call); if( e_ != hipSuccess ) { fd_gpu_fail( #call, e_ ); goto fail; } } while(0)

extern "C" char const * fd_ed25519_gpu_last_error( void ) { return fd_gpu_err; }
/* for the host units outside this file (fd_ed25519_gpu_unit.cpp) */
extern "C" void fd_ed25519_gpu_set_error( char const * what ) { snprintf( fd_gpu_err, sizeof(fd_gpu_err), "%s", what ); }

extern "C" int fd_ed25519_gpu_device_cnt( void ) {
  int cnt = 0;
  if( hipGetDeviceCount( &cnt ) != hipSuccess ) return 0;
  int ok = 0;
  for( int d=0; d<cnt; d++ ) {
    hipDeviceProp_t p;
    if( hipGetDeviceProperties( &p, d ) != hipSuccess ) continue;
    if( !strncmp( p.gcnArchName, "gfx950", 6 ) ) ok++;
  }
  return ok;
}

static void fd_work_carve( fd_ed25519_gpu_work_t * w, void * base, unsigned long N ) {
  uint8_t * p = (uint8_t *)base;
  w->tab      = (int32_t *)p; p += 4UL * FD_TAB_SIG * N;
  w->pts      = (int32_t *)p; p +=  320UL * N;
  w->fin      = (int32_t *)p; p +=  160UL * N;   /* 16-byte aligned rows: 1856 N is a multiple of 16 */
  w->status   = (int32_t *)p; p +=    4UL * N;
  w->pstat    = (int32_t *)p; p +=    8UL * N;
  w->op_start = (int32_t *)p; p +=    4UL * N;
  w->ops      = (uint8_t *)p; p += (unsigned long)FD_OPS_MAX * N;
  w->sdig     = (uint32_t *)p;                   /* FD_SDIG_BYTES, 16-byte aligned (every array above is) */
}

/* First use of a stream, not engine creation, pays for its queues: the
   first H2D copy, kernel and D2H copy on a fresh stream (a CU-masked one
   most of all) cost milliseconds -- the 8.7-9.1 ms maximum of the
   16-thread per-signature runs, when a third group-commit leader first
   used its slot (profiles/r04_in_direct_ab.jsonl).  Engine creation
   therefore sends copies of every size class each way and one blit
   kernel down every stream a batch can take. */
#define FD_WARM_MAX (16UL<<20)
static hipError_t fd_stream_warm( hipStream_t st, fd_ed25519_gpu_slot * sl, unsigned long cap, unsigned long max_sigs ) {
  hipError_t e;
  unsigned long osz = max_sigs * sizeof(int32_t) < 64UL ? max_sigs * sizeof(int32_t) : 64UL;   /* d_out / h_out hold max_sigs codes */
  unsigned long top = cap < FD_WARM_MAX ? cap : FD_WARM_MAX;
  for( unsigned long sz=64UL; ; sz<<=3 ) {
    if( sz > top ) sz = top;
    if( (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, sz, hipMemcpyHostToDevice, st )) != hipSuccess ) return e;
    if( sz == top ) break;
  }
  if( (e = hipMemsetAsync( sl->d_out, 0, osz, st )) != hipSuccess ) return e;
  if( (e = hipMemcpyAsync( sl->h_out, sl->d_out, osz, hipMemcpyDeviceToHost, st )) != hipSuccess ) return e;
  return hipStreamSynchronize( st );
}

/* (Re)create the slots' CU-masked streams: slot s runs on group s mod
   groups, a contiguous range of logical CUs (physically spread over all
   8 XCDs, disjoint from the other groups).
   groups <= 1 (or no CU masking on this runtime): every batch takes the
   whole device.  Slots must be idle. */
static void fd_cu_groups_make( fd_ed25519_gpu_t * g, int groups ) {
  for( int k=0; k<g->depth; k++ ) if( g->slot[k].mstream ) { hipStreamDestroy( g->slot[k].mstream ); g->slot[k].mstream = NULL; }
  int ncu = g->ncu, words = (ncu + 31) / 32;
  if( groups > g->depth ) groups = g->depth;
  if( groups < 1 || words > 32 || groups > ncu ) groups = 1;
  g->groups = groups;
  /* a batch fits its group at one quad-DSM wave (16 signatures) per SIMD */
  g->mask_max = groups > 1 ? 64UL * (unsigned long)(ncu / groups) : 0UL;
  for( int s=0; groups > 1 && s<g->depth; s++ ) {
    uint32_t mask[32] = { 0 };
    /* group k = logical CUs [k*ncu/groups, (k+1)*ncu/groups): measured on
       MI355X (tools/cu_mask_probe.hip, profiles/r02_cu_mask_probe.txt)
       such a mask puts a stream's waves on exactly ncu/groups physical CUs
       spread over all 8 XCDs, disjoint from the other groups'; the
       interleaved mask (CU c in group c mod groups) used before reached
       all 256 physical CUs from every group -- no isolation at all */
    for( int c=0; c<ncu; c++ ) if( c / (ncu / groups) == s % groups ) mask[c >> 5] |= 1u << (c & 31);
    if( hipExtStreamCreateWithCUMask( &g->slot[s].mstream, (uint32_t)words, mask ) != hipSuccess
        || fd_stream_warm( g->slot[s].mstream, &g->slot[s], g->blob_cap, g->max_sigs ) != hipSuccess ) {
      (void)hipGetLastError();
      for( int k=0; k<g->depth; k++ ) if( g->slot[k].mstream ) { hipStreamDestroy( g->slot[k].mstream ); g->slot[k].mstream = NULL; }
      g->mask_max = 0UL; g->groups = 1;
      return;
    }
  }
}

extern "C" fd_ed25519_gpu_t * fd_ed25519_gpu_new( int device, unsigned long max_sigs, unsigned long max_blob ) {
  return fd_ed25519_gpu_new_ex( device, max_sigs, max_blob, FD_GPU_DEPTH_DEFAULT );
}

extern "C" fd_ed25519_gpu_t * fd_ed25519_gpu_new_ex( int device, unsigned long max_sigs, unsigned long max_blob, int depth ) {
  if( !max_sigs || max_sigs > (1UL<<28) || max_blob > (1UL<<32) - FD_BLOB_PAD || depth < 1 || depth > FD_GPU_DEPTH_MAX ) {
    snprintf( fd_gpu_err, sizeof(fd_gpu_err), "fd_ed25519_gpu_new: bad capacity" );
    return NULL;
  }
  int cnt = 0;
  if( hipGetDeviceCount( &cnt ) != hipSuccess || device < 0 || device >= cnt ) {
    snprintf( fd_gpu_err, sizeof(fd_gpu_err), "fd_ed25519_gpu_new: no HIP device %d (count %d)", device, cnt );
    return NULL;
  }
  hipDeviceProp_t prop;
  if( hipGetDeviceProperties( &prop, device ) != hipSuccess || strncmp( prop.gcnArchName, "gfx950", 6 ) ) {
    snprintf( fd_gpu_err, sizeof(fd_gpu_err), "fd_ed25519_gpu_new: device %d is not gfx950", device );
    return NULL;
  }
  fd_ed25519_gpu_t * g = new fd_ed25519_gpu_t();
  g->pool_min = FD_DSM_POOL_MIN_DEFAULT;
  g->quad_max = FD_DSM_QUAD_MAX_DEFAULT;
  g->oct_max  = FD_DSM_OCT_MAX_DEFAULT;
  {
    /* the latency path's batches (the ring's 4,096, the per-signature
       group commits) take the direct write; larger ones the D2H copy,
       where its ~5 us is noise (tests/test_gpu_host.py
       checks the direct path at 40,000 too).  A/B: 0 = always the copy */
    char const * od = getenv( "FD_ED25519_GPU_OUT_DIRECT_MAX" );
    g->out_direct_max = od ? strtoul( od, NULL, 0 ) : 4096UL;
    /* A/B: 0 = every blocking poll waits for the completion event */
    char const * em = getenv( "FD_ED25519_GPU_EARLY_MAX" );
    g->early_max = em ? strtoul( em, NULL, 0 ) : FD_EARLY_MAX_DEFAULT;
  }
  g->device = device; g->max_sigs = max_sigs; g->max_blob = max_blob; g->next_ticket = 1; g->depth = depth;
  __atomic_store_n( &g->timeout_ns, FD_WAIT_TIMEOUT_NS_DEFAULT, __ATOMIC_RELAXED );
  { char const * ga = getenv( "FD_ED25519_GPU_GROUP_ALWAYS" ); g->group_always = ga && atoi( ga ); }  /* experiments */
  /* a slot's pinned and device blob buffers also hold the batch's
     descriptors, 16-aligned after the padded blob, so a batch is ONE H2D
     copy (a second small copy costs ~17 us of a ~0.75 ms 4096-signature
     round trip: its own transfer plus the copy-to-copy gap) */
  unsigned long blob_cap = fd_desc_off( max_blob ) + max_sigs * sizeof(fd_ed25519_gpu_desc_t);
  g->blob_cap = blob_cap;
  HIPCHK( hipSetDevice( device ) );
  HIPCHK( fd_ed25519_gpu_upload_tables() );
  for( int s=0; s<g->depth; s++ ) {
    fd_ed25519_gpu_slot * sl = &g->slot[s];
    HIPCHK( hipHostMalloc( (void **)&sl->h_blob, blob_cap, hipHostMallocDefault ) );
    HIPCHK( hipHostMalloc( (void **)&sl->h_desc, max_sigs * sizeof(fd_ed25519_gpu_desc_t), hipHostMallocMapped ) );
    if( hipHostGetDevicePointer( (void **)&sl->h_desc_dev, sl->h_desc, 0 ) != hipSuccess ) { (void)hipGetLastError(); sl->h_desc_dev = NULL; }
    /* codes of small batches are written by the kernels straight into
       h_out (fine-grained, mapped: no D2H copy, fd_ring_verify) */
    HIPCHK( hipHostMalloc( (void **)&sl->h_out,  max_sigs * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent ) );
    if( hipHostGetDevicePointer( (void **)&sl->h_out_dev, sl->h_out, 0 ) != hipSuccess ) { (void)hipGetLastError(); sl->h_out_dev = NULL; }
    HIPCHK( hipMalloc( (void **)&sl->d_blob, blob_cap ) );
    HIPCHK( hipMemset( sl->d_blob, 0, blob_cap ) );
    HIPCHK( hipMalloc( (void **)&sl->d_desc, max_sigs * sizeof(fd_ed25519_gpu_desc_t) ) );
    HIPCHK( hipMalloc( (void **)&sl->d_out,  max_sigs * sizeof(int32_t) ) );
    HIPCHK( hipMalloc( &sl->d_work_base, FD_ED25519_GPU_WORK_PER_SIG * max_sigs + FD_SDIG_BYTES ) );
    fd_work_carve( &sl->work, sl->d_work_base, max_sigs );
    HIPCHK( hipMemset( sl->work.sdig, 0, FD_SDIG_BYTES ) );   /* launch tags start at 1 */
    HIPCHK( hipStreamCreateWithFlags( &sl->stream, hipStreamNonBlocking ) );
    HIPCHK( hipEventCreateWithFlags( &sl->done, hipEventDisableTiming ) );
    sl->ticket = 0;
    memset( sl->h_blob, 0, blob_cap < FD_WARM_MAX ? blob_cap : FD_WARM_MAX );   /* the warm copies land zeros (d_blob stays zeroed) */
    HIPCHK( fd_stream_warm( sl->stream, sl, blob_cap, max_sigs ) );
  }
  /* CU groups for small ring batches.  A 4,096-signature batch on the
     latency schedule is lone waves (256 quad-DSM waves, 192 front-end
     waves); with several in flight, a batch's front end landed on the
     SIMDs of another batch's quad-DSM waves and ran at their pace (111 ->
     ~250 us, tools/lat_trace3.py, tools/front_stamps.py).  Up to
     FD_CU_GROUPS slots get disjoint CU groups (fd_cu_groups_make);
     batches up to 64 signatures per group CU (one quad wave per SIMD) run
     there while other ring batches are in flight, larger ones and lone
     batches on the whole device.  With groups that really are disjoint
     (round 2: the interleaved masks of round 1 isolated nothing), the C2
     ring at depth 8: 22.5 -> 26.3 M verifies/s at 5 in flight (p99 0.97
     -> 0.83 ms), 28.5 M/s at p99 0.92 ms with 6 (profiles/r02_cu_groups_contiguous_ab.txt). */
  g->ncu = prop.multiProcessorCount;
  {
    /* groups scale with the ring up to 4 (64 CUs = 256 SIMDs each, one
       4,096-signature quad-DSM batch at one wave per SIMD):
       tools/ring_sweep.py, profiles/r02_ring_sweep.jsonl */
    int groups = g->depth < FD_CU_GROUPS ? g->depth : FD_CU_GROUPS;
    char const * ev = getenv( "FD_ED25519_GPU_CU_GROUPS" );    /* experiments */
    if( ev ) groups = atoi( ev );
    fd_cu_groups_make( g, groups );
  }
  HIPCHK( hipStreamCreateWithFlags( &g->dev_sf, hipStreamNonBlocking ) );
  {
    /* the DSM stream at the highest priority: as the pool's waves retire,
       its own next waves are dispatched first and the next launch's front
       end only fills what it leaves idle (its last round) */
    int lo = 0, hi = 0;
    if( hipDeviceGetStreamPriorityRange( &lo, &hi ) != hipSuccess ) { (void)hipGetLastError(); lo = hi = 0; }
    char const * pe = getenv( "FD_ED25519_GPU_DSM_PRIO" );   /* experiments: 0 = default priority */
    if( pe && !atoi( pe ) ) hi = 0;
    HIPCHK( hipStreamCreateWithPriority( &g->dev_sb, hipStreamNonBlocking, hi ) );
  }
  for( int b=0; b<2; b++ ) {
    HIPCHK( hipMalloc( &g->d_dev_work_base[b], FD_ED25519_GPU_WORK_PER_SIG * max_sigs + FD_SDIG_BYTES ) );
    fd_work_carve( &g->dev_work[b], g->d_dev_work_base[b], max_sigs );
    HIPCHK( hipMemset( g->dev_work[b].sdig, 0, FD_SDIG_BYTES ) );
    HIPCHK( hipEventCreateWithFlags( &g->dev_in[b],    hipEventDisableTiming ) );
    HIPCHK( hipEventCreateWithFlags( &g->dev_front[b], hipEventDisableTiming ) );
    HIPCHK( hipEventCreateWithFlags( &g->dev_back[b],  hipEventDisableTiming ) );
    HIPCHK( hipEventRecord( g->dev_back[b], g->dev_sb ) );
  }
  for( int k=0; k<FD_EV_CNT; k++ ) HIPCHK( hipEventCreate( &g->kev[k] ) );
  return g;
fail:
  fd_ed25519_gpu_delete( g );
  return NULL;
}

static int fd_stream_query( void * st ) {
  hipError_t e = hipStreamQuery( (hipStream_t)st );
  return e == hipSuccess ? 1 : e == hipErrorNotReady ? 0 : -1;
}

static hipError_t fd_reg_release( void * host );

extern "C" void fd_ed25519_gpu_delete( fd_ed25519_gpu_t * g ) {
  if( !g ) return;
  hipSetDevice( g->device );
  /* drain every stream, all waits under ONE deadline (the engine timeout
     for the whole drain, not per stream: 2 x depth + 2 streams at 10 s
     each made a wedged teardown take minutes): if the device is wedged
     the engine's memory is leaked rather than freed under a running
     kernel */
  long to = fd_timeout( g ), t0 = fd_now_ns();
  hipStream_t sts[2*FD_GPU_DEPTH_MAX + 2];
  int ns = 0;
  for( int s=0; s<g->depth; s++ ) { sts[ns++] = g->slot[s].stream; sts[ns++] = g->slot[s].mstream; }
  sts[ns++] = g->dev_sf; sts[ns++] = g->dev_sb;
  for( int k=0; k<ns; k++ ) {
    if( !sts[k] ) continue;
    long left = to < 0 ? -1L : to - (fd_now_ns() - t0);
    if( to >= 0 && left < 0 ) left = 0;
    if( fd_wait_query( fd_stream_query, (void *)sts[k], FD_POLL_SPIN_NS, left ) != 1 ) {
      snprintf( fd_gpu_err, sizeof(fd_gpu_err), "fd_ed25519_gpu_delete: device %d did not drain; engine leaked", g->device );
      return;
    }
  }
  for( int k=0; k<FD_GPU_UNIT_CNT; k++ ) fd_gpu_unit_fini( g->unit[k] );
  for( int k=0; k<FD_REG_MAX; k++ ) if( g->reg[k].p ) fd_reg_release( (void *)g->reg[k].p );
  for( int s=0; s<g->depth; s++ ) {
    fd_ed25519_gpu_slot * sl = &g->slot[s];
    if( sl->mstream ) hipStreamDestroy( sl->mstream );
    if( sl->h_blob ) hipHostFree( sl->h_blob );
    if( sl->h_desc ) hipHostFree( sl->h_desc );
    if( sl->h_out  ) hipHostFree( sl->h_out );
    if( sl->h_dig  ) hipHostFree( sl->h_dig );
    if( sl->h_sgn  ) hipHostFree( sl->h_sgn );
    if( sl->h_res  ) hipHostFree( sl->h_res );
    if( sl->t_desc ) hipFree( sl->t_desc );
    if( sl->t_res  ) hipFree( sl->t_res );
    if( sl->d_blob ) hipFree( sl->d_blob );
    if( sl->d_desc ) hipFree( sl->d_desc );
    if( sl->d_out  ) hipFree( sl->d_out );
    if( sl->d_work_base ) hipFree( sl->d_work_base );
    if( sl->stream ) hipStreamDestroy( sl->stream );
    if( sl->done   ) hipEventDestroy( sl->done );
    for( int h=0; h<2; h++ ) if( sl->sha_ev[h] ) hipEventDestroy( sl->sha_ev[h] );
  }
  for( int i=0; i<FD_DEV_STATS_MAX; i++ )
    for( int k=0; k<FD_EV_CNT; k++ ) if( g->dev_ev[i][k] ) hipEventDestroy( g->dev_ev[i][k] );
  for( int b=0; b<2; b++ ) {
    if( g->dev_in[b]    ) hipEventDestroy( g->dev_in[b] );
    if( g->dev_front[b] ) hipEventDestroy( g->dev_front[b] );
    if( g->dev_back[b]  ) hipEventDestroy( g->dev_back[b] );
    if( g->d_dev_work_base[b] ) hipFree( g->d_dev_work_base[b] );
  }
  if( g->dev_sf ) hipStreamDestroy( g->dev_sf );
  if( g->dev_sb ) hipStreamDestroy( g->dev_sb );
  for( int k=0; k<FD_EV_CNT; k++ ) if( g->kev[k] ) hipEventDestroy( g->kev[k] );
  for( int b=0; b<2; b++ ) {
    fd_txn_set * ts = &g->txn_set[b];
    if( ts->meta  ) hipFree( ts->meta );
    if( ts->part  ) hipFree( ts->part );
    if( ts->desc  ) hipFree( ts->desc );
    if( ts->codes ) hipFree( ts->codes );
    if( ts->done  ) hipEventDestroy( ts->done );
  }
  if( g->d_txn_pk ) hipFree( g->d_txn_pk );
  if( g->h_txn_pk ) hipHostFree( g->h_txn_pk );
  for( int k=0; k<6; k++ ) if( g->txn_ev[k] ) hipEventDestroy( g->txn_ev[k] );
  for( int k=0; k<4; k++ ) if( g->txn_ring_ev[k] ) hipEventDestroy( g->txn_ring_ev[k] );
  delete g;
}

extern "C" int fd_ed25519_gpu_depth( fd_ed25519_gpu_t const * g ) { return g ? g->depth : 0; }

static void fd_reclaim_orphans( fd_ed25519_gpu_t * g );
extern "C" int fd_ed25519_gpu_set_cu_groups( fd_ed25519_gpu_t * g, int groups ) {
  if( !g || groups < 1 || groups > FD_GPU_DEPTH_MAX ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  /* a slot whose codes were taken early is idle for its caller: let it retire */
  for( int s=0; s<g->depth; s++ ) if( g->slot[s].retiring && fd_event_wait( g->slot[s].done, fd_timeout( g ) ) ) return FD_ED25519_ERR_GPU;
  fd_reclaim_orphans( g );
  for( int s=0; s<g->depth; s++ ) if( g->slot[s].ticket || g->slot[s].staged ) return FD_ED25519_ERR_ARG;   /* ring busy */
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  fd_cu_groups_make( g, groups );
  return 0;
}
extern "C" int fd_ed25519_gpu_cu_groups( fd_ed25519_gpu_t const * g ) { return g ? g->groups : 0; }

/* the schedule knobs are set under the engine lock and read under it:
   submitters, the device-resident path and the feeder thread may run
   concurrently with a setter */
struct fd_knobs { int mode; unsigned long pool_min, quad_max, oct_max; };
static fd_knobs fd_knobs_get( fd_ed25519_gpu_t const * g ) {
  std::lock_guard<fd_ring_lock> guard( const_cast<fd_ed25519_gpu_t *>( g )->lock );
  fd_knobs k = { g->mode, g->pool_min, g->quad_max, g->oct_max };
  return k;
}

/* Host regions the ring may DMA from directly (no staging copy): a batch
   whose blob lies inside one goes H2D straight from the caller's bytes
   (plus the descriptors from the slot's pinned buffer).  Registrations are
   process-wide and counted: several engines may register one region (one
   input dcache DMA'd by every engine of a multi-engine tile in place,
   fd_verify_tile_new_multi_inplace); the runtime registers it once
   (portable: every device) and unregisters it with the last engine. */
static std::mutex                                                      fd_reg_lock;
static std::map<void const *, std::pair<unsigned long, unsigned long>> fd_reg_cnt;   /* host -> (sz, engines) */

static hipError_t fd_reg_acquire( void * host, unsigned long sz ) {
  std::lock_guard<std::mutex> guard( fd_reg_lock );
  auto it = fd_reg_cnt.find( host );
  if( it != fd_reg_cnt.end() ) {
    if( it->second.first != sz ) return hipErrorInvalidValue;   /* the same start, another size: not shareable */
    it->second.second++;
    return hipSuccess;
  }
  hipError_t e = hipHostRegister( host, sz, hipHostRegisterPortable );
  if( e != hipSuccess ) { (void)hipGetLastError(); return e; }
  fd_reg_cnt[ host ] = std::make_pair( sz, 1UL );
  return hipSuccess;
}
static hipError_t fd_reg_release( void * host ) {
  std::lock_guard<std::mutex> guard( fd_reg_lock );
  auto it = fd_reg_cnt.find( host );
  if( it == fd_reg_cnt.end() ) return hipErrorHostMemoryNotRegistered;
  if( --it->second.second ) return hipSuccess;
  fd_reg_cnt.erase( it );
  hipError_t e = hipHostUnregister( host );
  if( e != hipSuccess ) (void)hipGetLastError();
  return e;
}

extern "C" int fd_ed25519_gpu_register( fd_ed25519_gpu_t * g, void * host, unsigned long sz ) {
  if( !g || !host || !sz ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  int k = 0;
  while( k<FD_REG_MAX && g->reg[k].p ) k++;
  if( k == FD_REG_MAX ) return FD_ED25519_ERR_ARG;
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  e = fd_reg_acquire( host, sz );
  if( e != hipSuccess ) return fd_gpu_fail( "hipHostRegister", e );
  g->reg[k].p = (uint8_t const *)host; g->reg[k].sz = sz;
  return 0;
}
extern "C" int fd_ed25519_gpu_unregister( fd_ed25519_gpu_t * g, void * host ) {
  if( !g || !host ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  for( int k=0; k<FD_REG_MAX; k++ ) if( g->reg[k].p == host ) {
    for( int s=0; s<g->depth; s++ ) {     /* no batch may still read from it */
      fd_ed25519_gpu_slot * sl = &g->slot[s];
      if( sl->ticket && fd_event_wait( sl->done, fd_timeout( g ) ) ) return FD_ED25519_ERR_GPU;
    }
    hipError_t e = fd_reg_release( host );
    g->reg[k].p = NULL; g->reg[k].sz = 0;
    return e == hipSuccess ? 0 : fd_gpu_fail( "hipHostUnregister", e );
  }
  return FD_ED25519_ERR_ARG;
}
static int fd_registered( fd_ed25519_gpu_t const * g, void const * p, unsigned long sz ) {
  uint8_t const * b = (uint8_t const *)p;
  for( int k=0; k<FD_REG_MAX; k++ )
    if( g->reg[k].p && b >= g->reg[k].p && sz <= g->reg[k].sz && (unsigned long)(b - g->reg[k].p) <= g->reg[k].sz - sz ) return 1;
  return 0;
}

extern "C" int fd_ed25519_gpu_set_timeout( fd_ed25519_gpu_t * g, long timeout_ns ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  __atomic_store_n( &g->timeout_ns, timeout_ns, __ATOMIC_RELAXED );
  return 0;
}
extern "C" long fd_ed25519_gpu_timeout( fd_ed25519_gpu_t const * g ) { return g ? fd_timeout( g ) : 0L; }

extern "C" int fd_ed25519_gpu_set_mode( fd_ed25519_gpu_t * g, int mode ) {
  if( !g || (mode != FD_ED25519_GPU_MODE_AVX && mode != FD_ED25519_GPU_MODE_PORTABLE && mode != FD_ED25519_GPU_MODE_STRICT) ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  g->mode = mode;
  return 0;
}
extern "C" int fd_ed25519_gpu_mode( fd_ed25519_gpu_t const * g ) { return g ? fd_knobs_get( g ).mode : -1; }
extern "C" int fd_ed25519_gpu_set_dsm_pool_min( fd_ed25519_gpu_t * g, unsigned long n ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  g->pool_min = n;
  return 0;
}
extern "C" unsigned long fd_ed25519_gpu_dsm_pool_min( fd_ed25519_gpu_t const * g ) { return g ? fd_knobs_get( g ).pool_min : 0UL; }
extern "C" int fd_ed25519_gpu_set_dsm_quad_max( fd_ed25519_gpu_t * g, unsigned long n ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  g->quad_max = n;
  return 0;
}
extern "C" unsigned long fd_ed25519_gpu_dsm_quad_max( fd_ed25519_gpu_t const * g ) { return g ? fd_knobs_get( g ).quad_max : 0UL; }
extern "C" int fd_ed25519_gpu_set_dsm_oct_max( fd_ed25519_gpu_t * g, unsigned long n ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  g->oct_max = n;
  return 0;
}
extern "C" unsigned long fd_ed25519_gpu_dsm_oct_max( fd_ed25519_gpu_t const * g ) { return g ? fd_knobs_get( g ).oct_max : 0UL; }
extern "C" unsigned long fd_ed25519_gpu_max_sigs( fd_ed25519_gpu_t const * g ) { return g ? g->max_sigs : 0UL; }
extern "C" unsigned long fd_ed25519_gpu_max_blob( fd_ed25519_gpu_t const * g ) { return g ? g->max_blob : 0UL; }

/* Slots orphaned by a timed-out wait (a synchronous call, or a staged
   per-signature chunk whose blocking poll gave up) come back once their
   event completes.  Caller holds g->lock. */
static void fd_reclaim_orphans( fd_ed25519_gpu_t * g ) {
  for( int s=0; s<g->depth; s++ ) {
    fd_ed25519_gpu_slot * sl = &g->slot[s];
    if( (sl->orphan || sl->retiring) && hipEventQuery( sl->done ) == hipSuccess ) {
      /* an orphan is nobody's: its stage (if the failing caller has not
         unstaged it yet) goes with it; a retiring slot keeps its owner's */
      if( sl->orphan ) sl->staged = 0;
      sl->orphan = 0; sl->retiring = 0; sl->ticket = 0; sl->n_txn = 0UL;
    }
  }
}

/* the slot holding ticket (never 0) / the slot whose pinned blob buffer is
   blob, or NULL.  Caller holds g->lock. */
static fd_ed25519_gpu_slot * fd_slot_by_ticket( fd_ed25519_gpu_t * g, unsigned long ticket ) {
  for( int s=0; s<g->depth; s++ ) if( g->slot[s].ticket == ticket ) return &g->slot[s];
  return NULL;
}
static fd_ed25519_gpu_slot * fd_slot_by_blob( fd_ed25519_gpu_t * g, void const * blob ) {
  for( int s=0; s<g->depth; s++ ) if( g->slot[s].h_blob == blob ) return &g->slot[s];
  return NULL;
}

/* Give up on a submitted ticket nobody will poll again (its blocking poll
   timed out): the slot is reclaimed by fd_reclaim_orphans once the batch
   drains, instead of staying taken for the engine's lifetime. */
static void fd_abandon_ticket( fd_ed25519_gpu_t * g, unsigned long ticket ) {
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl = fd_slot_by_ticket( g, ticket );
  if( sl ) sl->orphan = 1;
}

/* No slot is free, but one whose codes a poll took early is only retiring
   (its completion event follows within microseconds): wait for it and
   reclaim it, so a caller that submits right after such a poll finds the
   slot as it would have without the early return.  Caller holds g->lock.
   Returns 1 if a slot came back. */
/* the bound on that wait under the lock: a retiring slot's event follows
   its codes within microseconds (hundreds under a loaded device); one that
   has not fired within 2 ms (a wedged device) is left for later -- the
   caller sees a full ring -- rather than stalling every engine caller for
   the whole engine timeout */
#define FD_RETIRE_WAIT_NS 2000000L
static int fd_wait_retiring( fd_ed25519_gpu_t * g ) {
  for( int s=0; s<g->depth; s++ )
    if( g->slot[s].retiring ) {
      if( fd_wait_query( fd_event_query, (void *)g->slot[s].done, FD_RETIRE_WAIT_NS, FD_RETIRE_WAIT_NS ) != 1 ) return 0;
      fd_reclaim_orphans( g );
      return 1;
    }
  return 0;
}

/* Lend a free slot's pinned staging buffers (zero-copy submit). */
extern "C" int fd_ed25519_gpu_stage( fd_ed25519_gpu_t * g, void ** blob, fd_ed25519_gpu_desc_t ** desc ) {
  if( !g || !blob || !desc ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_reclaim_orphans( g );
  for( int pass=0; pass<2; pass++ ) {
    for( int s=0; s<g->depth; s++ ) {
      fd_ed25519_gpu_slot * sl = &g->slot[s];
      if( !sl->ticket && !sl->staged ) { sl->staged = 1; *blob = sl->h_blob; *desc = sl->h_desc; return 0; }
    }
    if( !fd_wait_retiring( g ) ) break;
  }
  return FD_ED25519_ERR_ARG;
}

/* A stage is released exactly once, by its owner: unstage, a submit of
   its blob, or a failed submit of it (which releases it under the same
   lock hold, so a slot orphaned by that failure is never seen staged by
   fd_reclaim_orphans and lent to a second caller while the first still
   holds it -- ADVICE r05). */
extern "C" void fd_ed25519_gpu_unstage( fd_ed25519_gpu_t * g, void const * blob ) {
  if( !g ) return;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl = fd_slot_by_blob( g, blob );
  if( sl ) sl->staged = 0;
}

/* a free slot: the staged one owning `blob` if any, else any unstaged one
   (slots orphaned by a timed-out synchronous call come back once done) */
static fd_ed25519_gpu_slot * fd_free_slot_( fd_ed25519_gpu_t * g, void const * blob ) {
  fd_reclaim_orphans( g );
  fd_ed25519_gpu_slot * own = fd_slot_by_blob( g, blob );
  if( own && !own->ticket ) return own;
  if( g->groups > 1 ) {
    /* slot s runs on CU group s mod groups: of the free slots, take one on
       the group with the fewest batches in flight, so a ring kept below
       its depth spreads its batches evenly over the groups; among those,
       the group whose newest batch is oldest (it frees its CUs first) */
    int cnt[FD_GPU_DEPTH_MAX] = { 0 };
    unsigned long newest[FD_GPU_DEPTH_MAX] = { 0 };
    for( int s=0; s<g->depth; s++ ) {
      unsigned long t = g->slot[s].ticket;
      if( t ) { cnt[s % g->groups]++; if( t > newest[s % g->groups] ) newest[s % g->groups] = t; }
    }
    int best = -1;
    for( int s=0; s<g->depth; s++ ) {
      if( g->slot[s].ticket || g->slot[s].staged ) continue;
      int k = s % g->groups, b = best < 0 ? 0 : best % g->groups;
      if( best < 0 || cnt[k] < cnt[b] || (cnt[k] == cnt[b] && newest[k] < newest[b]) ) best = s;
    }
    return best < 0 ? NULL : &g->slot[best];
  }
  for( int s=0; s<g->depth; s++ ) if( !g->slot[s].ticket && !g->slot[s].staged ) return &g->slot[s];
  return NULL;
}
static fd_ed25519_gpu_slot * fd_free_slot( fd_ed25519_gpu_t * g, void const * blob ) {
  fd_ed25519_gpu_slot * sl = fd_free_slot_( g, blob );
  if( !sl && fd_wait_retiring( g ) ) sl = fd_free_slot_( g, blob );
  return sl;
}

/* ---- The two slot lifecycles ----------------------------------------------

   A synchronous call: take -> stage -> enqueue -> settle, all under
   g->lock.  The call takes a free slot, stages its input in the slot's
   pinned blob, queues its own HIP work and the slot's done event on the
   slot's stream, and hands the outcome to fd_slot_settle, the one way out:
   no path returns with work queued on a slot that is neither waited for
   nor orphaned.

   A ring batch of either kind (fd_ring_submit, fd_ring_poll): take ->
   enqueue -> ticket under one hold of g->lock (a failed enqueue is settled
   as above; the stage submitted from is released either way), then polls,
   which wait outside the lock.  A poll that times out or is refused ends
   nothing: the ticket stays valid.  One that collects ends in
     free    the ticket is cleared;
     retire  a small batch's codes were taken as they landed: the slot keeps
             its ticket until fd_reclaim_orphans sees its done event;
     keep    either, and the pinned buffers stay the caller's until unstaged;
     orphan  (fd_abandon_ticket, for a caller that gives up) as retire, and
             a stage goes with the slot. */

/* Take: the device and a free slot (the staged one owning blob, if any).
   0, the fd_gpu_fail code, or FD_ED25519_ERR_ARG when every slot is in
   flight or lent out. */
static int fd_slot_take( fd_ed25519_gpu_t * g, void const * blob, fd_ed25519_gpu_slot ** sl ) {
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  return (*sl = fd_free_slot( g, blob )) ? 0 : FD_ED25519_ERR_ARG;
}

/* Stage: the blob into the slot's pinned buffer (unless it is that
   buffer), a second piece behind it (blob2_sz 0: none), zeros up to the
   16-aligned offset behind its pad, and the descriptors (or whatever
   travels in their place; NULL: the caller writes it there) at that
   offset, so the batch is one H2D copy.  Returns that offset. */
static unsigned long fd_slot_stage( fd_ed25519_gpu_slot * sl, void const * blob, unsigned long sz0, void const * blob2, unsigned long blob2_sz,
                                    void const * tail, unsigned long tail_sz ) {
  unsigned long blob_sz = sz0 + blob2_sz, doff = fd_desc_off( blob_sz );
  if( sl->h_blob != blob && sz0 ) memcpy( sl->h_blob, blob, sz0 );
  if( blob2_sz ) memcpy( sl->h_blob + sz0, blob2, blob2_sz );
  memset( sl->h_blob + blob_sz, 0, doff - blob_sz );
  if( tail ) memcpy( sl->h_blob + doff, tail, tail_sz );
  return doff;
}

/* Give up a slot whose done event is queued behind work still in flight:
   fd_reclaim_orphans brings it back once the event completes. */
static void fd_slot_orphan( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl ) {
  sl->ticket = g->next_ticket++; sl->orphan = 1;
}

/* Settle: the end of every synchronous call (err: what its enqueue on st
   returned) and of a failed ring enqueue.  Every wait is bounded by the
   engine's timeout, so a wedged stream never blocks the other users of
   the engine lock.  An enqueue that went through is waited for; one that
   failed may have left work on st (the H2D copy from the slot's pinned
   buffer, kernels on its scratch), which must drain before the slot can be
   picked again.  A wait that gives up leaves the slot orphaned behind its
   done event, and a slot that cannot even get that event is never reused
   (leaked).  Returns the error to hand back. */
static int fd_slot_settle( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, hipStream_t st, int err ) {
  if( !err ) {
    if( (err = fd_event_wait( sl->done, fd_timeout( g ) )) ) fd_slot_orphan( g, sl );
  } else if( st && fd_wait_query( fd_stream_query, (void *)st, FD_POLL_SPIN_NS, fd_timeout( g ) ) != 1 ) {
    /* the slot's done event marks the end of what was queued on st */
    if( hipEventRecord( sl->done, st ) == hipSuccess ) { fd_slot_orphan( g, sl ); sl->n_txn = 0UL; }
    else sl->ticket = ~0UL;
  }
  return err;
}

/* Scratch a call allocated for itself, after fd_slot_settle: while the
   slot is not free again (orphaned or leaked), queued work may still read
   or write the scratch, host or device, so it is left allocated and never
   freed -- a leak bounded by the number of timeouts. */
static inline int fd_slot_in_flight( fd_ed25519_gpu_slot const * sl ) { return sl->ticket != 0UL; }

extern "C" int fd_ed25519_gpu_device( fd_ed25519_gpu_t const * g ) { return g ? g->device : -1; }

extern "C" int fd_ed25519_gpu_slot_states( fd_ed25519_gpu_t * g, int * out, int max ) {
  if( !g || !out || max <= 0 ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  int k = 0;
  for( ; k<g->depth && k<max; k++ ) {
    fd_ed25519_gpu_slot const * sl = &g->slot[k];
    out[k] = ( sl->ticket ? 1 : 0 ) | ( sl->staged ? 2 : 0 ) | ( sl->retiring ? 4 : 0 ) | ( sl->orphan ? 8 : 0 )
           | ( sl->early ? 16 : 0 ) | ( hipEventQuery( sl->done ) == hipSuccess ? 32 : 0 );
  }
  (void)hipGetLastError();
  return k;
}

/* The device-resident path.  Descriptors are bounds-checked on the device
   against blob_sz (fd_k_prep reports FD_ED25519_ERR_ARG, nothing reads
   outside the blob).  Launch k takes working set b = k mod 2:
     stream: record dev_in[b]
     dev_sf: wait dev_in[b] (inputs ready), wait dev_back[b] (launch k-2
             done with set b); front part; record dev_front[b]
     dev_sb: wait dev_front[b]; back part (DSM, codes to d_out); record dev_back[b]
     stream: wait dev_back[b]
   so the caller's stream sees the codes in order, and launch k's front
   end overlaps launch k-1's DSM (its tail: the pool's last round of
   waves, ~0.9 ms per 1M-signature launch, tools/pool_rounds.py). */
static int fd_dev_launch( fd_ed25519_gpu_t * g, unsigned long n, void const * d_blob, unsigned long blob_sz,
                          fd_ed25519_gpu_desc_t const * d_desc, int * d_out, void * stream, int flags, fd_knobs const & kn ) {
  hipStream_t st = stream ? (hipStream_t)stream : g->slot[0].stream;
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  int b = (int)(g->dev_seq & 1UL);
  int mode = kn.mode;
  fd_ed25519_gpu_work_t const * w = &g->dev_work[b];
  hipEvent_t const * ev = NULL;
  if( g->dev_stats_on && g->dev_stats_cnt < FD_DEV_STATS_MAX ) {
    if( !g->dev_ev[g->dev_stats_cnt][0] )
      for( int k=0; k<FD_EV_CNT; k++ )
        if( (e = hipEventCreate( &g->dev_ev[g->dev_stats_cnt][k] )) != hipSuccess ) return fd_gpu_fail( "hipEventCreate", e );
    ev = g->dev_ev[g->dev_stats_cnt++];
  }
  /* inputs: ordered after the work already on the caller's stream --
     which includes its wait for the previous launch's codes, so the front
     end cannot start early -- unless the caller vouches that they are
     complete (FD_ED25519_GPU_DEV_INPUTS_READY), which lets this launch's
     front end overlap the previous launch's DSM */
  if( !(flags & FD_ED25519_GPU_DEV_INPUTS_READY) )
    if( (e = hipEventRecord( g->dev_in[b], st )) != hipSuccess
     || (e = hipStreamWaitEvent( g->dev_sf, g->dev_in[b], 0 )) != hipSuccess ) return fd_gpu_fail( "dev order (inputs)", e );
  if( (e = hipStreamWaitEvent( g->dev_sf, g->dev_back[b], 0 )) != hipSuccess ) return fd_gpu_fail( "dev order (front)", e );
  if( (e = fd_ed25519_gpu_launch_front( n, (uint8_t const *)d_blob, blob_sz, d_desc, w, g->dev_sf, ev, mode, kn.pool_min, kn.quad_max, kn.oct_max )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_front", e );
  if( (e = hipEventRecord( g->dev_front[b], g->dev_sf )) != hipSuccess
   || (e = hipStreamWaitEvent( g->dev_sb, g->dev_front[b], 0 )) != hipSuccess ) return fd_gpu_fail( "dev order (back)", e );
  if( (e = fd_ed25519_gpu_launch_back( n, (uint8_t const *)d_blob, d_desc, w, (int32_t *)d_out, g->dev_sb, ev, mode, kn.pool_min, kn.quad_max, kn.oct_max )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_back", e );
  if( (e = hipEventRecord( g->dev_back[b], g->dev_sb )) != hipSuccess
   || (e = hipStreamWaitEvent( st, g->dev_back[b], 0 )) != hipSuccess ) return fd_gpu_fail( "dev order (caller)", e );
  g->dev_seq++;
  return 0;
}

/* duration (ms) of kernel k of a launch timed with events ev[FD_EV_CNT]
   (fd_ed25519_gpu_private.h: the DSM from the back part's own start) */
static hipError_t fd_kernel_ms( float * ms, hipEvent_t const * ev, int k ) {
  return hipEventElapsedTime( ms, ev[k == 3 ? FD_EV_BACK : k], ev[k+1] );
}

/* Per-kernel durations of the pipelined launches issued between begin
   and end (at most FD_DEV_STATS_MAX), each kernel bracketed by HIP events
   on the stream it runs on -- measured while launches overlap, so a
   kernel's duration includes any slow-down from the next launch's front
   end sharing its SIMDs.  end() blocks until those launches are done and
   writes the per-kernel SUM (ms) in fd_ed25519_gpu_verify_dev_timed's
   phase order and the launch count. */
extern "C" int fd_ed25519_gpu_dev_stats_begin( fd_ed25519_gpu_t * g ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  std::lock_guard<std::mutex> guard( g->dev_lock );
  g->dev_stats_on = 1; g->dev_stats_cnt = 0;
  return 0;
}
extern "C" int fd_ed25519_gpu_dev_stats_end( fd_ed25519_gpu_t * g, float * kernel_ms_sum, unsigned long * launches ) {
  if( !g || !kernel_ms_sum || !launches ) return FD_ED25519_ERR_ARG;
  std::lock_guard<std::mutex> guard( g->dev_lock );
  g->dev_stats_on = 0;
  for( int k=0; k<FD_ED25519_GPU_KERNEL_CNT; k++ ) kernel_ms_sum[k] = 0.f;
  *launches = g->dev_stats_cnt;
  hipError_t e;
  for( unsigned long i=0; i<g->dev_stats_cnt; i++ ) {
    int err = fd_event_wait( g->dev_ev[i][FD_ED25519_GPU_KERNEL_CNT], fd_timeout( g ) );
    if( err ) return err;
    for( int k=0; k<FD_ED25519_GPU_KERNEL_CNT; k++ ) {
      float ms = 0.f;
      if( (e = fd_kernel_ms( &ms, g->dev_ev[i], k )) != hipSuccess ) return fd_gpu_fail( "elapsed", e );
      kernel_ms_sum[k] += ms;
    }
  }
  return 0;
}

/* the DSM kernels' clock accumulators (fd_dsm_clk, kernels.hip): clear, or
   read [waves, cycles, ticks] of the pool, quad and oct DSMs */
extern "C" hipError_t fd_ed25519_gpu_dsm_clk_xfer( unsigned long long * host, int clear );
extern "C" int fd_ed25519_gpu_dsm_clock( fd_ed25519_gpu_t * g, int clear, unsigned long long * out ) {
  if( !g || (!clear && !out) ) return FD_ED25519_ERR_ARG;
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  if( (e = fd_ed25519_gpu_dsm_clk_xfer( out, clear )) != hipSuccess ) return fd_gpu_fail( "dsm clock", e );
  return 0;
}

/* a serial device-resident operation on `st` using working set 0: waits
   for every earlier pipelined launch, and later ones wait for it */
static hipError_t fd_dev_serial_begin( fd_ed25519_gpu_t * g, hipStream_t st ) {
  hipError_t e;
  for( int b=0; b<2; b++ ) if( (e = hipStreamWaitEvent( st, g->dev_back[b], 0 )) != hipSuccess ) return e;
  return hipSuccess;
}
static hipError_t fd_dev_serial_end( fd_ed25519_gpu_t * g, hipStream_t st ) {
  hipError_t e;
  for( int b=0; b<2; b++ ) if( (e = hipEventRecord( g->dev_back[b], st )) != hipSuccess ) return e;
  return hipSuccess;
}

extern "C" int fd_ed25519_gpu_verify_dev_ex( fd_ed25519_gpu_t * g, unsigned long n, void const * d_blob, unsigned long blob_sz,
                                             fd_ed25519_gpu_desc_t const * d_desc, int * d_out, void * stream, int flags ) {
  /* the blob is the caller's device memory: max_blob (the pinned ring's
     capacity) does not bound it */
  if( !g || n > g->max_sigs || (n && (!d_blob || !d_desc || !d_out)) || (flags & ~FD_ED25519_GPU_DEV_INPUTS_READY) )
    return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  fd_knobs kn = fd_knobs_get( g );     /* before dev_lock: the engine's locks are never nested */
  std::lock_guard<std::mutex> guard( g->dev_lock );
  return fd_dev_launch( g, n, d_blob, blob_sz, d_desc, d_out, stream, flags, kn );
}

extern "C" int fd_ed25519_gpu_verify_dev( fd_ed25519_gpu_t * g, unsigned long n, void const * d_blob, unsigned long blob_sz,
                                          fd_ed25519_gpu_desc_t const * d_desc, int * d_out, void * stream ) {
  return fd_ed25519_gpu_verify_dev_ex( g, n, d_blob, blob_sz, d_desc, d_out, stream, 0 );
}

extern "C" int fd_ed25519_gpu_verify_dev_timed( fd_ed25519_gpu_t * g, unsigned long n, void const * d_blob, unsigned long blob_sz,
                                                fd_ed25519_gpu_desc_t const * d_desc, int * d_out, void * stream,
                                                float * kernel_ms ) {
  if( !g || n > g->max_sigs || !kernel_ms || (n && (!d_blob || !d_desc || !d_out)) ) return FD_ED25519_ERR_ARG;
  for( int k=0; k<FD_ED25519_GPU_KERNEL_CNT; k++ ) kernel_ms[k] = 0.f;
  if( !n ) return 0;
  fd_knobs kn = fd_knobs_get( g );     /* before dev_lock: the engine's locks are never nested */
  std::lock_guard<std::mutex> guard( g->dev_lock );
  /* serial, on the caller's stream, so each kernel's events bracket it alone */
  hipStream_t st = stream ? (hipStream_t)stream : g->slot[0].stream;
  hipError_t e0 = hipSetDevice( g->device );
  if( e0 != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e0 );
  int mode = kn.mode;
  if( (e0 = fd_dev_serial_begin( g, st )) != hipSuccess ) return fd_gpu_fail( "dev order", e0 );
  if( (e0 = fd_ed25519_gpu_launch_timed( n, (uint8_t const *)d_blob, blob_sz, d_desc, &g->dev_work[0], (int32_t *)d_out, st, g->kev,
                                         mode, kn.pool_min, kn.quad_max, kn.oct_max )) != hipSuccess ) return fd_gpu_fail( "fd_ed25519_gpu_launch", e0 );
  if( (e0 = fd_dev_serial_end( g, st )) != hipSuccess ) return fd_gpu_fail( "dev order", e0 );
  int err;
  if( (err = fd_event_wait( g->kev[FD_ED25519_GPU_KERNEL_CNT], fd_timeout( g ) )) ) return err;
  hipError_t e;
  for( int k=0; k<FD_ED25519_GPU_KERNEL_CNT; k++ )
    if( (e = fd_kernel_ms( &kernel_ms[k], g->kev, k )) != hipSuccess ) return fd_gpu_fail( "elapsed", e );
  return 0;
}

extern "C" int fd_ed25519_gpu_kernel_cnt( void ) { return FD_ED25519_GPU_KERNEL_CNT; }

/* The stream of a ring batch of n signatures: the slot's CU group only while
   another ring batch is in flight (a lone batch runs faster spread over
   the whole device: depth-1 p50 0.755 ms there vs 0.80 ms on a third of
   the CUs) */
static hipStream_t fd_ring_stream( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long n ) {
  int busy = 0;
  for( int s=0; s<g->depth && !busy; s++ )
    busy = &g->slot[s] != sl && g->slot[s].ticket && hipEventQuery( g->slot[s].done ) == hipErrorNotReady;
  int others = sl->mstream && n <= g->mask_max && (g->group_always || busy);
  return others ? sl->mstream : sl->stream;
}

/* Place: decide how the batch travels, and stage what must be staged.
   The batch's bytes are blob[0, sz0) followed by blob2[0, blob2_sz) (a
   second piece: an in-place batch that continues past the caller's ring
   wrap); descriptors index the concatenation.  tail: what travels behind
   the blob, at doff in the device's layout: the caller's descriptors
   (copied as given: the device checks each against blob_sz and reports an
   out-of-bounds one as FD_ED25519_ERR_ARG, fd_k_prep), or NULL where the
   caller builds it at the returned .tail (a transaction batch's entries and
   claim prefix) -- it lies nowhere yet, so it is never direct or packed. */
struct fd_ring_src {
  void const *  blob, * blob2;
  unsigned long sz0, blob2_sz, doff, tail_sz;
  uint8_t *     tail;
  int           direct, packed, zc;
};
static fd_ring_src fd_ring_place( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, void const * blob, unsigned long sz0,
                                  void const * blob2, unsigned long blob2_sz, void const * tail, unsigned long tail_sz ) {
  fd_ring_src p = { blob, blob2, sz0, blob2_sz, fd_desc_off( sz0 + blob2_sz ), tail_sz, (uint8_t *)sl->h_desc, 0, 0, 0 };
  /* a blob in a registered region is DMA'd from where it lies (no host
     copy; the tail goes separately from the slot's pinned desc buffer);
     anything else (the slot's own staged h_blob as it lies) is staged into
     the slot's pinned buffer with the tail packed after it (one copy) */
  p.direct = sl->h_blob != blob && sz0 && fd_registered( g, blob, sz0 ) && ( !blob2_sz || fd_registered( g, blob2, blob2_sz ) );
  /* descriptors in a registered region too go from where they lie (a
     verify tile building batches in its own registered buffers) */
  int const tdirect = p.direct && tail && fd_registered( g, tail, tail_sz );
  /* ... and packed right after the blob in the device's layout: one copy */
  p.packed = tdirect && !blob2_sz && (uint8_t const *)tail == (uint8_t const *)blob + p.doff && fd_registered( g, blob, p.doff + tail_sz );
  /* a registered span whose tail lies elsewhere (the feeder rebases
     descriptors; an in-place tile keeps them apart from the frags; a
     transaction batch's 12 bytes per transaction are built here): the
     kernels read it over PCIe from the slot's mapped descriptor buffer
     instead of a second H2D copy per batch (closed loop +1-2.5 %, p50
     -0.01 ms, profiles/r06_zc_desc_ab_*.jsonl) */
  p.zc = p.direct && !p.packed && sl->h_desc_dev;
  if( !p.direct ) p.tail = sl->h_blob + fd_slot_stage( sl, blob, sz0, blob2, blob2_sz, tail, tail_sz );
  else if( tdirect && !p.zc ) p.tail = (uint8_t *)tail;
  else if( tail ) memcpy( p.tail, tail, tail_sz );
  return p;
}

/* Copy in, on st: one copy of the staged batch or of the caller's packed
   region; else the blob, piece 2 and (unless the kernels read it in place)
   the tail.  Returns the tail as the kernels address it, NULL on failure. */
static void const * fd_ring_h2d( fd_ed25519_gpu_slot * sl, fd_ring_src const & p, hipStream_t st ) {
  hipError_t e;
  if( p.packed || !p.direct ) e = hipMemcpyAsync( sl->d_blob, p.packed ? p.blob : sl->h_blob, p.doff + p.tail_sz, hipMemcpyHostToDevice, st );
  else {
    e = hipMemcpyAsync( sl->d_blob, p.blob, p.sz0, hipMemcpyHostToDevice, st );
    if( e == hipSuccess && p.blob2_sz ) e = hipMemcpyAsync( sl->d_blob + p.sz0, p.blob2, p.blob2_sz, hipMemcpyHostToDevice, st );
    if( e == hipSuccess && !p.zc )      e = hipMemcpyAsync( sl->d_blob + p.doff, p.tail, p.tail_sz, hipMemcpyHostToDevice, st );
  }
  if( e != hipSuccess ) { fd_gpu_fail_q( p.direct ? "H2D batch (registered)" : "H2D batch", e ); return NULL; }
  return p.zc ? (void const *)sl->h_desc_dev : (void const *)( sl->d_blob + p.doff );
}

/* Verify: the launch on the slot's work area.  Up to out_direct_max
   signatures the DSM writes its codes into the slot's pinned h_out itself:
   no D2H copy (a blit kernel and its gap, ~5 us of every small batch's
   round trip); they are visible to the host once the slot's done event
   completes -- or, with early set, to a poll as they land over
   FD_CODE_PENDING (fd_codes_query).  Returns where they go, or NULL. */
static int32_t * fd_ring_verify( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long n, unsigned long blob_sz,
                                 void const * d_desc, hipStream_t st, int early ) {
  int odirect = sl->h_out_dev && n <= g->out_direct_max;
  int32_t * codes = odirect ? sl->h_out_dev : sl->d_out;
  sl->early = early && odirect && n <= g->early_max;
  if( sl->early ) for( unsigned long i=0; i<n; i++ ) sl->h_out[i] = FD_CODE_PENDING;
  hipError_t e = fd_ed25519_gpu_launch( n, sl->d_blob, blob_sz, (fd_ed25519_gpu_desc_t const *)d_desc, &sl->work, codes, st,
                                        g->mode, g->pool_min, g->quad_max, g->oct_max );
  if( e != hipSuccess ) { fd_gpu_fail_q( "launch", e ); return NULL; }
  return codes;
}

/* Finish: the codes to h_out where the DSM did not write them there, and
   the slot's done event */
static int fd_ring_finish( fd_ed25519_gpu_slot * sl, unsigned long n, int32_t const * codes, hipStream_t st ) {
  hipError_t e = codes == sl->d_out ? hipMemcpyAsync( sl->h_out, sl->d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, st ) : hipSuccess;
  if( e == hipSuccess ) e = hipEventRecord( sl->done, st );
  return e == hipSuccess ? 0 : fd_gpu_fail( "D2H out, event", e );
}

/* A descriptor batch: copy-in, kernels, copy-out on the slot's stream */
static int fd_slot_enqueue_( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long n, void const * blob,
                             unsigned long blob_sz, void const * blob2, unsigned long blob2_sz,
                             fd_ed25519_gpu_desc_t const * desc, hipStream_t * used ) {
  fd_ring_src p = fd_ring_place( g, sl, blob, blob_sz, blob2, blob2_sz, desc, n * sizeof(fd_ed25519_gpu_desc_t) );
  hipStream_t st = *used = fd_ring_stream( g, sl, n );
  void const * dd = fd_ring_h2d( sl, p, st );
  int32_t * codes = dd ? fd_ring_verify( g, sl, n, blob_sz + blob2_sz, dd, st, 1 ) : NULL;
  if( !codes || fd_ring_finish( sl, n, codes, st ) ) return FD_ED25519_ERR_GPU;
  sl->n = n; sl->n_txn = 0UL;
  return 0;
}

/* a finished batch's results (res: a transaction batch's); NULL: not wanted */
static void fd_slot_collect( fd_ed25519_gpu_slot * sl, int * codes, fd_ed25519_gpu_txn_result_t * res ) {
  if( res ) memcpy( res, sl->h_res, sl->n_txn * sizeof(fd_ed25519_gpu_txn_result_t) );
  if( codes && sl->n ) memcpy( codes, sl->h_out, sl->n * sizeof(int) );
}

extern "C" int fd_ed25519_gpu_verify_packed( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                             fd_ed25519_gpu_desc_t const * desc, int * out ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && (!desc || !out)) || (blob_sz && !blob) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  /* use a free slot; synchronous callers serialise on the lock */
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  hipStream_t st = NULL;
  err = fd_slot_enqueue_( g, sl, n, blob, blob_sz, NULL, 0UL, desc, &st );
  if( (err = fd_slot_settle( g, sl, st, err )) ) return err;
  fd_slot_collect( sl, out, NULL );
  return 0;
}

/* Submit a ring batch of either kind: ensure() (what the kind needs
   allocated: 0 or the error), a free slot, enqueue( sl, &st ), the ticket.
   1 submitted, 0 the ring is full (poll first), < 0 an error. */
template< class Ensure, class Enqueue >
static int fd_ring_submit( fd_ed25519_gpu_t * g, void const * blob, unsigned long * ticket, Ensure ensure, Enqueue enqueue ) {
  std::lock_guard<fd_ring_lock> guard( g->lock );
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  int err = ensure();
  if( err ) return err;
  fd_ed25519_gpu_slot * sl = fd_free_slot( g, blob );
  if( !sl ) return 0;
  hipStream_t st = NULL;
  err = enqueue( sl, &st );
  if( err ) err = fd_slot_settle( g, sl, st, err );
  sl->staged = 0;                        /* released, submitted or not (fd_ed25519_gpu_unstage) */
  if( err ) return err;
  *ticket = sl->ticket = g->next_ticket++;
  return 1;
}

/* what the submits that do not wait for a slot return: a full ring is the caller's error */
static inline int fd_submit_code( int r ) { return r == 1 ? 0 : r == 0 ? FD_ED25519_ERR_ARG : r; }

extern "C" int fd_ed25519_gpu_try_submit2( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                           void const * blob2, unsigned long blob2_sz,
                                           fd_ed25519_gpu_desc_t const * desc, unsigned long * ticket ) {
  if( !g || !ticket || n > g->max_sigs || blob_sz > g->max_blob || blob2_sz > g->max_blob - blob_sz || (n && !desc)
      || (blob_sz && !blob) || (blob2_sz && !blob2) ) return FD_ED25519_ERR_ARG;
  return fd_ring_submit( g, blob, ticket, []{ return 0; }, [&]( fd_ed25519_gpu_slot * sl, hipStream_t * st ) {
    return fd_slot_enqueue_( g, sl, n, blob, blob_sz, blob2, blob2_sz, desc, st );
  } );
}

extern "C" int fd_ed25519_gpu_try_submit( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                          fd_ed25519_gpu_desc_t const * desc, unsigned long * ticket ) {
  return fd_ed25519_gpu_try_submit2( g, n, blob, blob_sz, NULL, 0UL, desc, ticket );
}

extern "C" int fd_ed25519_gpu_submit( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                      fd_ed25519_gpu_desc_t const * desc, unsigned long * ticket ) {
  return fd_submit_code( fd_ed25519_gpu_try_submit( g, n, blob, blob_sz, desc, ticket ) );
}

/* A small direct-output batch's codes, each written once by the DSM into
   the slot's coherent pinned h_out over FD_CODE_PENDING: all in means the
   batch's results are final although the kernel may still be retiring (its
   completion event, a marker behind it, reaches the host some microseconds
   later).  Returns 1 all codes in, 2 the event completed, -1 a failed
   query; the event is queried only every 16th call. */
struct fd_codes_ctx { fd_ed25519_gpu_slot * sl; unsigned it; };
static int fd_codes_query( void * p ) {
  fd_codes_ctx * c = (fd_codes_ctx *)p;
  volatile int32_t const * o = c->sl->h_out;
  unsigned long i = 0, n = c->sl->n;
  while( i < n && o[i] != FD_CODE_PENDING ) i++;
  if( i == n ) { __atomic_thread_fence( __ATOMIC_ACQUIRE ); return 1; }
  if( (c->it++ & 15u) ) return 0;
  int r = fd_event_query( (void *)c->sl->done );
  return r == 1 ? 2 : r;
}

/* Poll a ticket: res set wants a transaction ticket (codes optional), codes
   alone a descriptor ticket -- the other kind's is refused and stays valid
   -- and neither is a drain, which takes either kind.  1 collected, 0 in
   flight (non-blocking), < 0 timed out or failed: the ticket stays valid. */
static int fd_ring_poll( fd_ed25519_gpu_t * g, unsigned long ticket, int block, int * codes, fd_ed25519_gpu_txn_result_t * res ) {
  fd_ed25519_gpu_slot * sl;
  {
    std::lock_guard<fd_ring_lock> guard( g->lock );
    sl = fd_slot_by_ticket( g, ticket );
    if( !sl || ( (codes || res) && !res != !sl->n_txn ) ) return FD_ED25519_ERR_ARG;
  }
  int landed = 0;   /* the codes are in ahead of the event: the slot comes back once that completes */
  if( (block & 1) && sl->early && codes ) {   /* a drain waits for the event */
    fd_codes_ctx c = { sl, 1u };
    int r = fd_batch_wait( fd_codes_query, &c, fd_timeout( g ), "" );
    if( r < 0 ) return r;
    landed = r == 1;
  } else if( block & 1 ) {
    int err = fd_event_wait( sl->done, fd_timeout( g ) );
    if( err ) return err;
  } else {
    hipError_t e = hipEventQuery( sl->done );
    if( e == hipErrorNotReady ) return 0;
    if( e != hipSuccess ) return fd_gpu_fail( "poll", e );
  }
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_slot_collect( sl, codes, res );
  sl->early = 0;
  if( landed ) sl->retiring = 1;
  else { sl->ticket = 0; sl->n_txn = 0UL; }
  if( block & FD_ED25519_GPU_POLL_KEEP ) sl->staged = 1;   /* its pinned buffers stay the caller's (unstage to free) */
  return 1;
}

extern "C" int fd_ed25519_gpu_poll( fd_ed25519_gpu_t * g, unsigned long ticket, int * out, int block ) {
  if( !g || !ticket ) return FD_ED25519_ERR_ARG;
  return fd_ring_poll( g, ticket, block, out, NULL );
}

/* Diagnostics: the device field products (fd_k_debug_fe, ops 0-6; op 7
   the oct DSM's half product, fd_k_debug_oct) over n
   operand pairs f, g ([n][10] int32 limbs); h receives [3][n][10] limbs.
   Synchronous; host buffers; n <= 2^20. */
extern "C" int fd_ed25519_gpu_debug_fe( fd_ed25519_gpu_t * g, int op, unsigned long n, int const * f, int const * gg, int * h ) {
  if( !g || op < 0 || op > 7 || n > (1UL<<20) || (n && (!f || !gg || !h)) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  hipError_t e;
  hipStream_t st = sl->stream;
  unsigned long sz = 40UL * n;
  int32_t * d = NULL;
  if( (e = hipMalloc( (void **)&d, 5UL * sz )) != hipSuccess ) return fd_gpu_fail( "debug_fe alloc", e );
  if( (e = hipMemcpyAsync( d, f, sz, hipMemcpyHostToDevice, st )) != hipSuccess
   || (e = hipMemcpyAsync( d + 10UL*n, gg, sz, hipMemcpyHostToDevice, st )) != hipSuccess
   || (e = fd_ed25519_gpu_launch_debug_fe( op, n, d, d + 10UL*n, d + 20UL*n, st )) != hipSuccess
   || (e = hipMemcpyAsync( h, d + 20UL*n, 3UL * sz, hipMemcpyDeviceToHost, st )) != hipSuccess
   || (e = hipEventRecord( sl->done, st )) != hipSuccess ) err = fd_gpu_fail( "debug_fe", e );
  err = fd_slot_settle( g, sl, st, err );
  if( !fd_slot_in_flight( sl ) ) hipFree( d );
  return err;
}

/* n 64-byte digests as the SHA-512 state words fd_k_prep_dig takes: digest
   byte 8j+b becomes bits 56-8b.. of word j */
static void fd_dig_words( uint64_t * w, uint8_t const * dig, unsigned long n ) {
  for( unsigned long i=0; i<8UL*n; i++ ) {
    uint64_t x = 0UL;
    for( int b=0; b<8; b++ ) x = (x << 8) | (uint64_t)dig[8UL*i + (unsigned long)b];
    w[i] = x;
  }
}

/* the device's k words [4][n] as n x 32 little-endian bytes: zeros where
   prep's status is not 1 (no k was computed) */
static void fd_k_bytes( uint8_t * k_out, uint64_t const * h_k, int32_t const * h_st, unsigned long n ) {
  for( unsigned long i=0; i<n; i++ )
    for( int j=0; j<4; j++ ) {
      uint64_t w = h_st[i] == 1 ? h_k[(unsigned long)j*n + i] : 0UL;
      for( int b=0; b<8; b++ ) k_out[32UL*i + 8UL*(unsigned long)j + (unsigned long)b] = (uint8_t)(w >> (8*b));
    }
}

/* Diagnostics: k = SHA-512(R||A||M) mod L of each signature, computed by
   fd_k_prep on the device (the SURVEY.md section 7 minimum-slice check:
   compared with the reference's fd_sha512_* + fd_ed25519_sc_reduce,
   fd_ed25519_user.c:411-414).  k_out receives n x 32 bytes; signatures
   the S check settles (and malformed descriptors) get 32 zero bytes and
   status_out[i] != 1 (the reference computes no k for them either).
   Synchronous; host buffers. */
extern "C" int fd_ed25519_gpu_debug_k( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                       fd_ed25519_gpu_desc_t const * desc, uint8_t * k_out, int * status_out ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && (!desc || !k_out || !status_out)) || (blob_sz && !blob) )
    return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  /* the only place both engine locks are held: dev_lock first, as every
     device-resident path takes it (none of them takes g->lock while
     holding it: their knobs are read before), so no two threads can wait
     on each other's lock */
  std::lock_guard<std::mutex> dguard( g->dev_lock );
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  hipError_t e;
  hipStream_t st = sl->stream;
  unsigned long doff = fd_slot_stage( sl, blob, blob_sz, NULL, 0UL, desc, n * sizeof(fd_ed25519_gpu_desc_t) );
  uint64_t * d_k = (uint64_t *)g->dev_work[0].tab;   /* 1536 B of table scratch per signature >= 32 */
  uint8_t * h = (uint8_t *)malloc( 36UL * n );       /* k [4][n], status [n] */
  if( !h ) return FD_ED25519_ERR_GPU;
  uint64_t * h_k = (uint64_t *)h;
  int32_t * h_st = (int32_t *)(h + 32UL * n);
  if( (e = fd_dev_serial_begin( g, st )) != hipSuccess
   || (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, doff + n * sizeof(fd_ed25519_gpu_desc_t), hipMemcpyHostToDevice, st )) != hipSuccess
   || (e = hipMemsetAsync( d_k, 0, 32UL * n, st )) != hipSuccess
   || (e = fd_ed25519_gpu_launch_prep_k( n, sl->d_blob, blob_sz, (fd_ed25519_gpu_desc_t const *)(sl->d_blob + doff), &g->dev_work[0], d_k, st )) != hipSuccess
   || (e = hipMemcpyAsync( h_k, d_k, 32UL * n, hipMemcpyDeviceToHost, st )) != hipSuccess
   || (e = hipMemcpyAsync( h_st, g->dev_work[0].status, 4UL * n, hipMemcpyDeviceToHost, st )) != hipSuccess
   || (e = hipEventRecord( sl->done, st )) != hipSuccess
   || (e = fd_dev_serial_end( g, st )) != hipSuccess ) err = fd_gpu_fail( "debug_k", e );
  if( err ) (void)fd_dev_serial_end( g, st );   /* best effort: later device-resident launches still wait for what was queued */
  if( !(err = fd_slot_settle( g, sl, st, err )) ) {
    memcpy( status_out, h_st, 4UL * n );
    fd_k_bytes( k_out, h_k, h_st, n );
  }
  if( !fd_slot_in_flight( sl ) ) free( h );
  return err;
}

static int fd_diag_run( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                        fd_ed25519_gpu_desc_t const * desc, uint8_t const * dig, int with_k,
                        int * codes_out, uint8_t * k_out, int * status_out, int * pstat_out, int * pts_out,
                        int * op_start_out, uint8_t * ops_out, int * tab_out, int * fin_out, int * info_out );

/* Diagnostics: the verify pipeline with each signature's 64-byte digest
   given by the caller (dig, n x 64 bytes: what the reference hands to
   fd_ed25519_sc_reduce, fd_ed25519_user.c:411-414) in place of
   SHA-512(R||A||M) -- so k is the caller's choice and a test can build a
   valid signature at any (S, k).  Everything else is the product path: S
   check, decompression, small-order flags, the DSM of the schedule the
   engine's mode and knobs give a batch of n (as fd_ed25519_gpu_launch_front
   / _back choose it), compare, code precedence, ERR_ARG for descriptors
   outside the blob.  The message bytes are not read.  fd_k_prep_dig takes
   SHA-512 state words, so digest byte 8j+b becomes bits 56-8b.. of word j.
   codes_out receives n codes; k_out (n x 32 bytes) and status_out as in
   fd_ed25519_gpu_debug_k, either may be NULL.  Synchronous; host buffers. */
extern "C" int fd_ed25519_gpu_debug_verify_dig( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                                fd_ed25519_gpu_desc_t const * desc, uint8_t const * dig, int * codes_out,
                                                uint8_t * k_out, int * status_out ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && (!desc || !dig || !codes_out)) || (blob_sz && !blob) )
    return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  return fd_diag_run( g, n, blob, blob_sz, desc, dig, 1, codes_out, k_out, status_out, NULL, NULL, NULL, NULL, NULL, NULL, NULL );
}

/* Diagnostics: one verify launch with the stages it leaves in the working
   set (dev_work[0]) read back -- prep's status, the point statuses and
   decompressed points, the op streams, the Ai tables and the pooled DSM's
   final p1p1 rows -- each in one layout whatever the schedule's own (see
   fd_ed25519_gpu_diag.h).  dig NULL: the product's front
   (fd_ed25519_gpu_launch_front, real SHA-512); else
   fd_ed25519_gpu_launch_front_dig as fd_ed25519_gpu_debug_verify_dig.
   Host code only: the kernels run as in any other launch. */
extern "C" int fd_ed25519_gpu_debug_stages( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                            fd_ed25519_gpu_desc_t const * desc, uint8_t const * dig,
                                            int * codes_out, int * status_out, int * pstat_out, int * pts_out,
                                            int * op_start_out, uint8_t * ops_out, int * tab_out, int * fin_out,
                                            int * info_out ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && !desc) || (blob_sz && !blob) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  return fd_diag_run( g, n, blob, blob_sz, desc, dig, 0, codes_out, NULL, status_out, pstat_out, pts_out, op_start_out, ops_out,
                      tab_out, fin_out, info_out );
}

/* The core of the two: take, stage, one serial launch on dev_work[0] with
   scratch of its own, settle, unpack.  with_k (dig given): fd_k_prep_dig
   also leaves k, which k_out (if not NULL) receives as
   fd_ed25519_gpu_debug_k's.  Every out pointer may be NULL. */
static int fd_diag_run( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                        fd_ed25519_gpu_desc_t const * desc, uint8_t const * dig, int with_k,
                        int * codes_out, uint8_t * k_out, int * status_out, int * pstat_out, int * pts_out,
                        int * op_start_out, uint8_t * ops_out, int * tab_out, int * fin_out, int * info_out ) {
  fd_knobs kn = fd_knobs_get( g );     /* before the locks below: fd_knobs_get takes g->lock itself */
  /* the schedule, by fd_ed25519_gpu_launch_front's and _back's predicates */
  int const portable = (kn.mode & 0xff) == FD_ED25519_GPU_MODE_PORTABLE;
  int const pooled   = n >= kn.pool_min;
  int const oct      = !pooled && !portable && n <= kn.oct_max;
  int const quad     = !pooled && !portable && n <= kn.quad_max;
  int const sched    = pooled ? FD_ED25519_GPU_SCHED_POOLED : oct ? FD_ED25519_GPU_SCHED_OCT
                     : quad ? FD_ED25519_GPU_SCHED_QUAD : FD_ED25519_GPU_SCHED_UNIFORM;
  int const sigmajor = oct || quad;    /* the latency front end's signature-major op rows */
  int const has_tab  = !sigmajor;      /* fd_k_dsm (AoS per signature) or fd_k_dsm_setup ([entry][n]) */
  /* both engine locks, dev_lock first (fd_ed25519_gpu_debug_k) */
  std::lock_guard<std::mutex> dguard( g->dev_lock );
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  hipError_t e;
  hipStream_t st = sl->stream;
  unsigned long doff = fd_slot_stage( sl, blob, blob_sz, NULL, 0UL, desc, n * sizeof(fd_ed25519_gpu_desc_t) );
  fd_ed25519_gpu_desc_t const * d_desc = (fd_ed25519_gpu_desc_t const *)(sl->d_blob + doff);
  fd_ed25519_gpu_work_t const * w = &g->dev_work[0];
  /* device scratch: state words [n][8], k [4][n] (with_k), codes [n] (the
     working set's table scratch is the DSM's here); the host copy holds the
     stages behind them, each only if asked for */
  unsigned long const o_k = 64UL * n, o_c = o_k + ( with_k ? 32UL * n : 0UL ), dsz = o_c + 4UL * n;
  unsigned long o = dsz;
  unsigned long const o_st  = o; o += 4UL * n;
  unsigned long const o_ps  = o; o += pstat_out    ? 8UL * n : 0UL;
  unsigned long const o_os  = o; o += op_start_out ? 4UL * n : 0UL;
  unsigned long const o_pts = o; o += pts_out      ? 320UL * n : 0UL;
  unsigned long const o_fin = o; o += fin_out && pooled ? 160UL * n : 0UL;
  unsigned long const o_ops = o; o += ops_out      ? (unsigned long)FD_OPS_MAX * n : 0UL;
  unsigned long const o_tab = o; o += tab_out && has_tab ? 4UL * (unsigned long)FD_TAB_SIG * n : 0UL;
  uint8_t * h = (uint8_t *)malloc( o );
  uint8_t * d = NULL;
  if( !h ) return FD_ED25519_ERR_GPU;
  if( (e = hipMalloc( (void **)&d, dsz )) != hipSuccess ) { free( h ); return fd_gpu_fail( "debug_stages alloc", e ); }
  if( dig ) fd_dig_words( (uint64_t *)h, dig, n );
  if( (e = fd_dev_serial_begin( g, st )) != hipSuccess
   || (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, doff + n * sizeof(fd_ed25519_gpu_desc_t), hipMemcpyHostToDevice, st )) != hipSuccess
   || (dig && (e = hipMemcpyAsync( d, h, 64UL * n, hipMemcpyHostToDevice, st )) != hipSuccess)
   || (with_k && (e = hipMemsetAsync( d + o_k, 0, 32UL * n, st )) != hipSuccess)
   || (e = hipMemsetAsync( d + o_c, 0x7f, 4UL * n, st )) != hipSuccess       /* no code: a row the DSM left unwritten shows */
   || (e = dig ? fd_ed25519_gpu_launch_front_dig( n, sl->d_blob, blob_sz, d_desc, (uint64_t const *)d, w,
                                                  with_k ? (uint64_t *)(d + o_k) : (uint64_t *)NULL, st,
                                                  kn.mode, kn.pool_min, kn.quad_max, kn.oct_max )
               : fd_ed25519_gpu_launch_front( n, sl->d_blob, blob_sz, d_desc, w, st, NULL,
                                              kn.mode, kn.pool_min, kn.quad_max, kn.oct_max )) != hipSuccess
   || (e = hipMemcpyAsync( h + o_st, w->status, 4UL * n, hipMemcpyDeviceToHost, st )) != hipSuccess   /* prep's, before the DSM settles it */
   || (e = fd_ed25519_gpu_launch_back( n, sl->d_blob, d_desc, w, (int32_t *)(d + o_c), st, NULL,
                                       kn.mode, kn.pool_min, kn.quad_max, kn.oct_max )) != hipSuccess
   || (e = hipMemcpyAsync( h + o_k, d + o_k, dsz - o_k, hipMemcpyDeviceToHost, st )) != hipSuccess   /* k (with_k) and the codes */
   || (pstat_out    && (e = hipMemcpyAsync( h + o_ps,  w->pstat,    8UL * n,   hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (op_start_out && (e = hipMemcpyAsync( h + o_os,  w->op_start, 4UL * n,   hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (pts_out      && (e = hipMemcpyAsync( h + o_pts, w->pts,      320UL * n, hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (o_ops != o_fin && (e = hipMemcpyAsync( h + o_fin, w->fin,    160UL * n, hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (ops_out      && (e = hipMemcpyAsync( h + o_ops, w->ops, (unsigned long)FD_OPS_MAX * n, hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (o != o_tab   && (e = hipMemcpyAsync( h + o_tab, w->tab, 4UL * (unsigned long)FD_TAB_SIG * n, hipMemcpyDeviceToHost, st )) != hipSuccess)
   || (e = hipEventRecord( sl->done, st )) != hipSuccess
   || (e = fd_dev_serial_end( g, st )) != hipSuccess ) err = fd_gpu_fail( "debug_stages", e );
  if( err ) (void)fd_dev_serial_end( g, st );   /* as fd_ed25519_gpu_debug_k */
  if( (err = fd_slot_settle( g, sl, st, err )) ) {
    if( !fd_slot_in_flight( sl ) ) { hipFree( d ); free( h ); }
    return err;
  }
  if( codes_out )    memcpy( codes_out,    h + o_c,  4UL * n );
  if( status_out )   memcpy( status_out,   h + o_st, 4UL * n );
  if( k_out )        fd_k_bytes( k_out, (uint64_t const *)(h + o_k), (int32_t const *)(h + o_st), n );
  if( pstat_out )    memcpy( pstat_out,    h + o_ps, 8UL * n );
  if( op_start_out ) memcpy( op_start_out, h + o_os, 4UL * n );
  if( pts_out ) {      /* device: [40][2n] -> [2n][40] */
    int32_t const * s = (int32_t const *)(h + o_pts);
    for( unsigned long j=0; j<2UL*n; j++ )
      for( unsigned long k=0; k<40UL; k++ ) pts_out[40UL*j + k] = s[k*2UL*n + j];
  }
  if( ops_out ) {      /* device: [n][FD_OPS_MAX] (latency front end) or step-major [FD_OPS_MAX][n] */
    uint8_t const * s = h + o_ops;
    if( sigmajor ) memcpy( ops_out, s, (unsigned long)FD_OPS_MAX * n );
    else
      for( unsigned long i=0; i<n; i++ )
        for( unsigned long t=0; t<(unsigned long)FD_OPS_MAX; t++ ) ops_out[(unsigned long)FD_OPS_MAX*i + t] = s[t*n + i];
  }
  if( tab_out && has_tab ) {   /* device: [n][8][48] (fd_k_dsm) or [8][n][48] (fd_k_dsm_setup) */
    int32_t const * s = (int32_t const *)(h + o_tab);
    if( !pooled ) memcpy( tab_out, s, 4UL * (unsigned long)FD_TAB_SIG * n );
    else
      for( unsigned long i=0; i<n; i++ )
        for( unsigned long en=0; en<8UL; en++ )
          memcpy( tab_out + i*(unsigned long)FD_TAB_SIG + en*(unsigned long)FD_TAB_ENTRY,
                  s + (en*n + i)*(unsigned long)FD_TAB_ENTRY, 4UL * (unsigned long)FD_TAB_ENTRY );
  }
  if( fin_out && pooled ) memcpy( fin_out, h + o_fin, 160UL * n );
  if( info_out ) { info_out[0] = sched; info_out[1] = sigmajor; info_out[2] = has_tab; info_out[3] = pooled; }
  hipFree( d );
  free( h );
  return 0;
}

/* SHA-512 / SHA-384 of n messages blob[msg_off..+msg_sz) (sig_off and
   pub_off unused) on the device; hash_out receives n digests of 64 (48)
   bytes back to back.  Synchronous. */
extern "C" int fd_ed25519_gpu_sha512_packed( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                             fd_ed25519_gpu_desc_t const * desc, void * hash_out, int is384 ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && (!desc || !hash_out)) || (blob_sz && !blob) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  for( unsigned long i=0; i<n; i++ )
    if( (unsigned long)desc[i].msg_off + (unsigned long)desc[i].msg_sz > blob_sz ) return FD_ED25519_ERR_ARG;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, blob, &sl );
  if( err ) return err;
  hipError_t e;
  hipStream_t st = sl->stream;
  if( !sl->h_dig && (e = hipHostMalloc( (void **)&sl->h_dig, g->max_sigs * 64UL, hipHostMallocDefault )) != hipSuccess )
    return fd_gpu_fail( "hipHostMalloc digests", e );
  if( sl->h_blob != blob ) memcpy( sl->h_blob, blob, blob_sz );
  memset( sl->h_blob + blob_sz, 0, FD_BLOB_PAD );
  if( sl->h_desc != desc ) memcpy( sl->h_desc, desc, n * sizeof(fd_ed25519_gpu_desc_t) );
  void * d_dig = sl->work.tab;   /* 1536 B per signature of scratch >= 64 B per message */
  if(      (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, blob_sz + FD_BLOB_PAD, hipMemcpyHostToDevice, st )) != hipSuccess ) err = fd_gpu_fail( "H2D blob", e );
  else if( (e = hipMemcpyAsync( sl->d_desc, sl->h_desc, n * sizeof(fd_ed25519_gpu_desc_t), hipMemcpyHostToDevice, st )) != hipSuccess ) err = fd_gpu_fail( "H2D desc", e );
  else if( (e = fd_ed25519_gpu_launch_sha512( n, sl->d_blob, sl->d_desc, d_dig, is384, st )) != hipSuccess ) err = fd_gpu_fail( "launch sha512", e );
  else if( (e = hipMemcpyAsync( sl->h_dig, d_dig, n * 64UL, hipMemcpyDeviceToHost, st )) != hipSuccess ) err = fd_gpu_fail( "D2H digests", e );
  else if( (e = hipEventRecord( sl->done, st )) != hipSuccess ) err = fd_gpu_fail( "event", e );
  if( (err = fd_slot_settle( g, sl, st, err )) ) return err;
  unsigned long hsz = is384 ? 48UL : 64UL;
  for( unsigned long i=0; i<n; i++ ) memcpy( (uint8_t *)hash_out + i*hsz, sl->h_dig + i*64UL, hsz );
  sl->staged = 0;
  return 0;
}

/* ------------------------------------------------------------------ */
/* Process-default engine and the reference-shaped APIs. */

static std::mutex          fd_default_lock;
static fd_ed25519_gpu_t *  fd_default_gpu = NULL;
static unsigned long       fd_default_sigs = 1UL << 16;
static unsigned long       fd_default_blob = 1UL << 26;   /* $FD_ED25519_GPU_DEFAULT_BLOB overrides */

static fd_ed25519_gpu_t * fd_default_engine( void );
extern "C" fd_ed25519_gpu_t * fd_ed25519_gpu_default( void ) { return fd_default_engine(); }
/* group-commit leaders of fd_ed25519_verify = the default engine's ring
   depth (experiments: FD_ED25519_GPU_VQ_LEADERS, 1..FD_GPU_DEPTH_MAX).
   4: on the round-5 kernels (one box, profiles/r05_vq_leaders_ab.jsonl)
   64 native threads 83.3-84.0 K calls/s at 3 leaders against 90.4 K at 4
   (p99 1.08 ms) and 86.4 K at 5 (p99 1.22); 4 threads 8.8-9.0 K at p99
   0.62-0.67 ms against 10.8 K at p99 0.40; one thread unchanged. */
#define FD_VQ_LEADERS_DEFAULT 4
static int fd_vq_leaders( void ) {
  static int n = 0;
  if( !n ) {
    char const * e = getenv( "FD_ED25519_GPU_VQ_LEADERS" );
    int v = e ? atoi( e ) : FD_VQ_LEADERS_DEFAULT;
    n = v < 1 ? 1 : v > FD_GPU_DEPTH_MAX ? FD_GPU_DEPTH_MAX : v;
  }
  return n;
}

/* The default engine is released at exit, ahead of the HIP runtime's own
   teardown (its destructors were registered when it loaded, so they run
   after this handler): left to the runtime's teardown, its streams and
   pinned buffers crashed process exit under rocprofv3
   (profiles/r03_per_signature_timeline.json). */
static void fd_default_engine_fini( void ) {
  std::lock_guard<std::mutex> guard( fd_default_lock );
  fd_ed25519_gpu_t * g = fd_default_gpu;
  fd_default_gpu = NULL;
  /* the process is ending: drain for at most 2 s, then leave the memory to
     the process teardown rather than hold up exit */
  if( g ) {
    long to = fd_timeout( g );
    if( to < 0 || to > 2000000000L ) __atomic_store_n( &g->timeout_ns, 2000000000L, __ATOMIC_RELAXED );
    fd_ed25519_gpu_delete( g );
  }
}

static fd_ed25519_gpu_t * fd_default_engine( void ) {
  std::lock_guard<std::mutex> guard( fd_default_lock );
  if( !fd_default_gpu ) {
    char const * dev = getenv( "FD_ED25519_GPU_DEVICE" );
    char const * bl  = getenv( "FD_ED25519_GPU_DEFAULT_BLOB" );   /* staging blob bytes (messages above it take the long path) */
    unsigned long blob = bl ? strtoul( bl, NULL, 0 ) : fd_default_blob;
    if( blob < 4096UL ) blob = 4096UL;
    fd_default_gpu = fd_ed25519_gpu_new_ex( dev ? atoi( dev ) : 0, fd_default_sigs, blob, fd_vq_leaders() );
    static int fini_set = 0;
    if( fd_default_gpu && !fini_set ) { fini_set = 1; atexit( fd_default_engine_fini ); }
  }
  return fd_default_gpu;
}

/* stage() polled until a slot is free, bounded by the engine timeout */
static int fd_stage_wait( fd_ed25519_gpu_t * g, void ** blob, fd_ed25519_gpu_desc_t ** desc ) {
  long to = fd_timeout( g ), t0 = fd_now_ns();
  while( fd_ed25519_gpu_stage( g, blob, desc ) ) {
    long dt = fd_now_ns() - t0;
    if( to >= 0 && dt > to ) {
      snprintf( fd_gpu_err, sizeof(fd_gpu_err), "no free ring slot after %ld ms", to / 1000000L );
      return FD_ED25519_ERR_GPU;
    }
    if( dt <= FD_POLL_SPIN_NS ) __builtin_ia32_pause();
    else { struct timespec ts = { 0, 20000L }; nanosleep( &ts, NULL ); }
  }
  return 0;
}

/* ---- Long messages ------------------------------------------------------

   The reference verifies a message of any length: fd_sha512_append streams
   it (src/ballet/sha512/fd_sha512.c:282-349; fd_ed25519.h:96-101 bounds
   nothing).  A message too large for one staging blob (or for a 32-bit
   descriptor) is verified here without CPU crypto: the padded byte stream
   R || A || M || 0x80 || 0.. || bitlen is moved through a staged slot's
   pinned blob in pieces, each piece hashed on the device into a chaining
   state that stays in the slot's HBM between launches
   (fd_k_sha512_stream, one lane per message, several messages side by
   side), then the signatures run prep (digest from the state), point
   decompression and the uniform DSM (fd_ed25519_gpu_launch_long) -- the
   same code path bit for bit as any other batch after the hash.  SHA-512
   is serial within a message: one lane hashes ~1 GB/s / 64, so this is
   correct for any length but slow for very long messages. */
struct fd_long_req { uint8_t const * sig; uint8_t const * pub; uint8_t const * msg; unsigned long sz; };

/* bytes [pos, pos+len) of request r's padded SHA-512 input stream */
static void fd_long_pack( uint8_t * dst, fd_long_req const & r, unsigned long pos, unsigned long len ) {
  unsigned long T = 64UL + r.sz;                            /* R || A || M */
  unsigned long P = ( T + 17UL + 127UL ) & ~127UL;          /* padded */
  unsigned long x = pos, end = pos + len;
  if( x < 32UL && x < end ) { unsigned long k = ( end < 32UL ? end : 32UL ) - x; memcpy( dst, r.sig + x, k ); dst += k; x += k; }
  if( x < 64UL && x < end ) { unsigned long k = ( end < 64UL ? end : 64UL ) - x; memcpy( dst, r.pub + (x - 32UL), k ); dst += k; x += k; }
  if( x < T && x < end )    { unsigned long k = ( end < T ? end : T ) - x;       memcpy( dst, r.msg + (x - 64UL), k ); dst += k; x += k; }
  if( x < end ) {
    memset( dst, 0, end - x );
    if( x == T ) dst[0] = 0x80;                             /* the padding bit */
    if( end == P ) {                                        /* the 128-bit big-endian bit count ends the stream */
      uint8_t * L = dst + ( end - x ) - 16;
      unsigned long hi = T >> 61, lo = T << 3;
      for( int b=0; b<8; b++ ) { L[7-b] = (uint8_t)(hi >> (8*b)); L[15-b] = (uint8_t)(lo >> (8*b)); }
    }
  }
}

/* the staged slot owning blob (the caller holds the stage) */
static fd_ed25519_gpu_slot * fd_slot_of( fd_ed25519_gpu_t * g, void const * blob ) {
  std::lock_guard<fd_ring_lock> guard( g->lock );
  return fd_slot_by_blob( g, blob );
}

/* wait for the staged slot's queued work; on a timeout the slot is given
   up (orphaned: reclaimed once its event fires) instead of reused */
static int fd_long_wait( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl ) {
  hipError_t e = hipEventRecord( sl->done, sl->stream );
  if( e != hipSuccess ) return fd_gpu_fail( "long: event", e );
  int err = fd_event_wait( sl->done, fd_timeout( g ) );
  if( err ) {
    std::lock_guard<fd_ring_lock> guard( g->lock );
    fd_slot_orphan( g, sl ); sl->staged = 0;
  }
  return err;
}

static int fd_run_long( fd_ed25519_gpu_t * g, unsigned long cnt, fd_long_req const * rq, int * out ) {
  void * vb; fd_ed25519_gpu_desc_t * dd;
  int err = fd_stage_wait( g, &vb, &dd );
  if( err ) return err;
  fd_ed25519_gpu_slot * sl = fd_slot_of( g, vb );
  if( !sl ) { fd_ed25519_gpu_unstage( g, vb ); return FD_ED25519_ERR_GPU; }
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) { fd_ed25519_gpu_unstage( g, vb ); return fd_gpu_fail( "hipSetDevice", e ); }
  int mode = fd_knobs_get( g ).mode;
  uint64_t * d_st = (uint64_t *)sl->work.fin;              /* 160 B of scratch per signature >= the 64 B state */
  /* messages per group: each needs >= one 128-byte block and a 16-byte
     piece entry per launch, and its 96 bytes of R || S || A after */
  unsigned long G = g->max_blob / 256UL;
  if( G > g->max_sigs ) G = g->max_sigs;
  if( G > 4096UL ) G = 4096UL;
  if( !G ) { fd_ed25519_gpu_unstage( g, vb ); return FD_ED25519_ERR_ARG; }
  for( unsigned long i0=0; i0<cnt && !err; i0+=G ) {
    unsigned long m = cnt - i0 < G ? cnt - i0 : G;
    /* blocks per message per launch, the piece table after the data */
    unsigned long C = ( g->max_blob - m * sizeof(fd_sha_piece_t) ) / ( m * 128UL );
    unsigned long toff = m * C * 128UL;
    std::vector<unsigned long> pos( m, 0UL );
    for(;;) {
      fd_sha_piece_t * pc = (fd_sha_piece_t *)( sl->h_blob + toff );
      int more = 0;
      for( unsigned long j=0; j<m; j++ ) {
        fd_long_req const & r = rq[ i0 + j ];
        unsigned long P = ( 64UL + r.sz + 17UL + 127UL ) & ~127UL;
        unsigned long nb = ( P - pos[j] ) / 128UL;
        if( nb > C ) nb = C;
        pc[j].off = j * C * 128UL; pc[j].nblk = (uint32_t)nb; pc[j].first = pos[j] == 0UL;
        if( nb ) { fd_long_pack( sl->h_blob + j * C * 128UL, r, pos[j], nb * 128UL ); pos[j] += nb * 128UL; more = 1; }
      }
      if( !more ) break;
      if( (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, toff + m * sizeof(fd_sha_piece_t), hipMemcpyHostToDevice, sl->stream )) != hipSuccess
       || (e = fd_ed25519_gpu_launch_sha512_stream( (uint32_t)m, d_st, sl->d_blob, (fd_sha_piece_t const *)( sl->d_blob + toff ), sl->stream )) != hipSuccess ) {
        err = fd_gpu_fail( "long: hash piece", e ); break;
      }
      if( (err = fd_long_wait( g, sl )) ) return err;       /* the pinned blob is reused next round */
    }
    if( err ) break;
    /* the signatures: R || S || A per message, descriptors after */
    unsigned long bsz = 96UL * m, doff = fd_desc_off( bsz );
    fd_ed25519_gpu_desc_t * hd = (fd_ed25519_gpu_desc_t *)( sl->h_blob + doff );
    for( unsigned long j=0; j<m; j++ ) {
      memcpy( sl->h_blob + 96UL*j, rq[ i0 + j ].sig, 64 );
      memcpy( sl->h_blob + 96UL*j + 64UL, rq[ i0 + j ].pub, 32 );
      hd[j].sig_off = (uint32_t)(96UL*j); hd[j].pub_off = (uint32_t)(96UL*j + 64UL); hd[j].msg_off = 0; hd[j].msg_sz = 0;
    }
    memset( sl->h_blob + bsz, 0, doff - bsz );
    if( (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, doff + m * sizeof(fd_ed25519_gpu_desc_t), hipMemcpyHostToDevice, sl->stream )) != hipSuccess
     || (e = fd_ed25519_gpu_launch_long( m, sl->d_blob, bsz, (fd_ed25519_gpu_desc_t const *)( sl->d_blob + doff ), d_st, &sl->work,
                                         sl->d_out, sl->stream, mode )) != hipSuccess
     || (e = hipMemcpyAsync( sl->h_out, sl->d_out, m * sizeof(int32_t), hipMemcpyDeviceToHost, sl->stream )) != hipSuccess ) {
      err = fd_gpu_fail( "long: verify", e ); break;
    }
    if( (err = fd_long_wait( g, sl )) ) return err;
    for( unsigned long j=0; j<m; j++ ) out[ i0 + j ] = sl->h_out[j];
  }
  if( err ) (void)hipStreamSynchronize( sl->stream );      /* a failed enqueue: what was queued drains before the slot is lent again */
  fd_ed25519_gpu_unstage( g, vb );
  return err;
}

/* ---- Long plain hashes ---------------------------------------------------

   SHA-512 / SHA-384 of messages too large for a staging blob (or a 32-bit
   descriptor): the reference's batch API has no restriction on sz
   (src/ballet/sha256/fd_sha256.h:191-192).  As the long verify path above,
   the padded stream moves through a staged slot's pinned blob in pieces
   and the chaining states stay in the slot's work.fin rows; unlike it, the
   last piece of a message leaves its digest, big endian, in its row
   (fd_k_sha512_pieces), so one D2H copy per group and a memcpy per message
   deliver the results.  With FD_SHA_LONG_PINGPONG the blob is two halves
   (fd_sha512_gpu_pack.h) and the host packs one while the device hashes
   the other; the library ships the single buffer, which measured no slower
   (fd_sha512_gpu_private.h). */

/* the kernel that read a half has finished, so the half may be repacked;
   on a timeout the slot is given up as in fd_long_wait, its done event
   queued behind what is still in flight (if even that fails the slot stays
   staged: lost to the engine rather than lent out under a running kernel) */
static int fd_sha_half_wait( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, hipEvent_t ev ) {
  int err = fd_event_wait( ev, fd_timeout( g ) );
  if( err && hipEventRecord( sl->done, sl->stream ) == hipSuccess ) {
    std::lock_guard<fd_ring_lock> guard( g->lock );
    fd_slot_orphan( g, sl ); sl->staged = 0;
  }
  return err;
}

extern "C" int fd_sha512_gpu_long( fd_ed25519_gpu_t * g, unsigned long cnt, fd_sha_long_req_t const * rq, int is384 ) {
  if( !g ) return FD_ED25519_ERR_GPU;
  if( !cnt ) return 0;
  fd_sha_long_geom_t geo;
  (void)fd_sha_long_geom( g->max_blob, g->max_sigs, 1UL, FD_SHA_LONG_PINGPONG, &geo );
  unsigned long const G = geo.G;
  if( !G ) {
    snprintf( fd_gpu_err, sizeof(fd_gpu_err), "long hash: a blob of %lu bytes cannot hold one 128-byte block and its piece entry", g->max_blob );
    return FD_ED25519_ERR_ARG;
  }
  void * vb; fd_ed25519_gpu_desc_t * dd;
  int err = fd_stage_wait( g, &vb, &dd );
  if( err ) return err;
  fd_ed25519_gpu_slot * sl = fd_slot_of( g, vb );
  if( !sl ) { fd_ed25519_gpu_unstage( g, vb ); return FD_ED25519_ERR_GPU; }
  hipError_t e = hipSetDevice( g->device );
  /* the slot's two events and its pinned digests come with its first long hash (as h_dig with the first packed one) */
  for( int h=0; h<2 && e == hipSuccess; h++ ) if( !sl->sha_ev[h] ) e = hipEventCreateWithFlags( &sl->sha_ev[h], hipEventDisableTiming );
  if( e == hipSuccess && !sl->h_dig ) e = hipHostMalloc( (void **)&sl->h_dig, g->max_sigs * 64UL, hipHostMallocDefault );
  if( e != hipSuccess ) { fd_ed25519_gpu_unstage( g, vb ); return fd_gpu_fail( "long hash: setup", e ); }
  uint64_t * d_st = (uint64_t *)sl->work.fin;              /* 160 B of scratch per signature >= the 64 B row */
  uint32_t const fl = is384 ? FD_SHA_PIECE_384 : 0U;
  unsigned long const hsz = is384 ? 48UL : 64UL;
  std::vector<unsigned long> tot( G ), pos( G );           /* blocks of each stream, and how many are packed */
  for( unsigned long i0=0; i0<cnt && !err; i0+=G ) {
    unsigned long m = cnt - i0 < G ? cnt - i0 : G;
    (void)fd_sha_long_geom( g->max_blob, g->max_sigs, m, FD_SHA_LONG_PINGPONG, &geo );
    unsigned long C = geo.C, left = m, longest = 0UL;
    for( unsigned long j=0; j<m; j++ ) {
      tot[j] = fd_sha_long_blocks( rq[ i0 + j ].sz ); pos[j] = 0UL;
      if( tot[j] > longest ) longest = tot[j];
    }
    if( C > longest ) C = longest;                         /* a group of short streams copies no empty blocks */
    unsigned long const toff = m * C * 128UL, half_sz = toff + m * sizeof(fd_sha_lpiece_t);
    for( unsigned long launch=0; left; launch++ ) {
      unsigned long h = launch % geo.nhalf, off = h * half_sz;
      if( launch >= geo.nhalf && (err = fd_sha_half_wait( g, sl, sl->sha_ev[h] )) ) return err;
      fd_sha_lpiece_t * pc = (fd_sha_lpiece_t *)( sl->h_blob + off + toff );
      for( unsigned long j=0; j<m; j++ ) {
        fd_sha_long_req_t const & r = rq[ i0 + j ];
        unsigned long nb = tot[j] - pos[j];
        if( nb > C ) nb = C;
        pc[j].off = off + j * C * 128UL; pc[j].nblk = (uint32_t)nb;
        pc[j].flags = fl | ( pos[j] ? 0U : FD_SHA_PIECE_FIRST ) | ( pos[j] + nb == tot[j] ? FD_SHA_PIECE_LAST : 0U );
        if( nb ) {
          fd_sha_long_pack( sl->h_blob + off + j * C * 128UL, (uint8_t const *)r.data, r.sz, pos[j] * 128UL, nb * 128UL );
          pos[j] += nb;
          if( pos[j] == tot[j] ) left--;
        }
      }
      if( (e = hipMemcpyAsync( sl->d_blob + off, sl->h_blob + off, half_sz, hipMemcpyHostToDevice, sl->stream )) != hipSuccess
       || (e = fd_sha512_gpu_launch_pieces( (uint32_t)m, d_st, sl->d_blob, (fd_sha_lpiece_t const *)( sl->d_blob + off + toff ), sl->stream )) != hipSuccess
       || (e = hipEventRecord( sl->sha_ev[h], sl->stream )) != hipSuccess ) {
        err = fd_gpu_fail( "long hash: piece", e ); break;
      }
    }
    if( err ) break;
    if( (e = hipMemcpyAsync( sl->h_dig, d_st, m * 64UL, hipMemcpyDeviceToHost, sl->stream )) != hipSuccess ) {
      err = fd_gpu_fail( "long hash: D2H digests", e ); break;
    }
    if( (err = fd_long_wait( g, sl )) ) return err;
    for( unsigned long j=0; j<m; j++ ) memcpy( rq[ i0 + j ].hash, sl->h_dig + 64UL*j, hsz );
  }
  if( err ) (void)hipStreamSynchronize( sl->stream );      /* a failed enqueue: what was queued drains before the slot is lent again */
  fd_ed25519_gpu_unstage( g, vb );
  return err;
}

extern "C" int fd_sha512_gpu_long_geometry( unsigned long max_blob, unsigned long max_sigs, unsigned long m,
                                            unsigned long * G, unsigned long * C ) {
  fd_sha_long_geom_t geo;
  int r = fd_sha_long_geom( max_blob, max_sigs, m, FD_SHA_LONG_PINGPONG, &geo );
  if( G ) *G = geo.G;
  if( C ) *C = geo.C;
  return r ? FD_ED25519_ERR_ARG : 0;
}

/* Pack pointer-array inputs into a pinned slot blob in chunks of the
   engine capacity and run them: each chunk is staged in a free slot's
   pinned buffers, submitted and waited on through the ring (stage /
   try_submit / poll), so the engine lock is held only to take the slot,
   enqueue and collect -- never across the device round trip -- and
   callers on other threads run their batches on the other slots at the
   same time (fd_ed25519_verify's group-commit leaders).  Messages too long
   for a staging blob (or a 32-bit descriptor) take the long path. */
static int fd_run_ptr_short( fd_ed25519_gpu_t * g, unsigned long n, uint8_t const * const * msg, unsigned long const * msg_sz,
                             uint8_t const * shared_msg, unsigned long shared_sz,
                             uint8_t const * const * sigp, uint8_t const (*siga)[64],
                             uint8_t const * const * pubp, uint8_t const (*puba)[32], int * out );

static int fd_run_ptr_batch( fd_ed25519_gpu_t * g, unsigned long n, uint8_t const * const * msg, unsigned long const * msg_sz,
                             uint8_t const * shared_msg, unsigned long shared_sz,
                             uint8_t const * const * sigp, uint8_t const (*siga)[64],
                             uint8_t const * const * pubp, uint8_t const (*puba)[32], int * out ) {
  if( !g ) return FD_ED25519_ERR_GPU;
  unsigned long const lim = g->max_blob > 96UL ? g->max_blob - 96UL : 0UL;
  if( shared_msg ) {
    if( shared_sz <= lim && shared_sz <= 0x7fffffffUL ) return fd_run_ptr_short( g, n, NULL, NULL, shared_msg, shared_sz, sigp, siga, pubp, puba, out );
    std::vector<fd_long_req> rq( n );
    for( unsigned long k=0; k<n; k++ ) rq[k] = { sigp ? sigp[k] : siga[k], pubp ? pubp[k] : puba[k], shared_msg, shared_sz };
    return fd_run_long( g, n, rq.data(), out );
  }
  unsigned long nl = 0;
  for( unsigned long k=0; k<n; k++ ) nl += msg_sz[k] > lim || msg_sz[k] > 0x7fffffffUL;
  if( !nl ) return fd_run_ptr_short( g, n, msg, msg_sz, NULL, 0, sigp, siga, pubp, puba, out );
  /* split: the short ones through the ring as usual, the long ones after */
  std::vector<uint8_t const *> sm, ss, sp; std::vector<unsigned long> sz, si, li;
  std::vector<fd_long_req> rq;
  for( unsigned long k=0; k<n; k++ ) {
    uint8_t const * s = sigp ? sigp[k] : siga[k], * p = pubp ? pubp[k] : puba[k];
    if( msg_sz[k] > lim || msg_sz[k] > 0x7fffffffUL ) { rq.push_back( { s, p, msg[k], msg_sz[k] } ); li.push_back( k ); }
    else { sm.push_back( msg[k] ); sz.push_back( msg_sz[k] ); ss.push_back( s ); sp.push_back( p ); si.push_back( k ); }
  }
  std::vector<int> o( n );
  int err = si.empty() ? 0 : fd_run_ptr_short( g, si.size(), sm.data(), sz.data(), NULL, 0, ss.data(), NULL, sp.data(), NULL, o.data() );
  if( err ) return err;
  for( unsigned long j=0; j<si.size(); j++ ) out[ si[j] ] = o[j];
  if( (err = fd_run_long( g, rq.size(), rq.data(), o.data() )) ) return err;
  for( unsigned long j=0; j<li.size(); j++ ) out[ li[j] ] = o[j];
  return 0;
}

static int fd_run_ptr_short( fd_ed25519_gpu_t * g, unsigned long n, uint8_t const * const * msg, unsigned long const * msg_sz,
                             uint8_t const * shared_msg, unsigned long shared_sz,
                             uint8_t const * const * sigp, uint8_t const (*siga)[64],
                             uint8_t const * const * pubp, uint8_t const (*puba)[32], int * out ) {
  unsigned long i = 0;
  while( i < n ) {
    void * vb; fd_ed25519_gpu_desc_t * dd;
    int err = fd_stage_wait( g, &vb, &dd );
    if( err ) return err;
    uint8_t * hb = (uint8_t *)vb;
    /* fill one chunk (the slot is ours while staged) */
    unsigned long used = 0, cnt = 0;
    unsigned long shared_off = 0;
    if( shared_msg ) { memcpy( hb, shared_msg, shared_sz ); used = shared_sz; }
    while( i + cnt < n && cnt < g->max_sigs ) {
      unsigned long k = i + cnt;
      unsigned long msz = shared_msg ? 0UL : msg_sz[k];
      if( used + 96UL + msz > g->max_blob ) break;
      fd_ed25519_gpu_desc_t * d = &dd[cnt];
      d->sig_off = (uint32_t)used; memcpy( hb + used, sigp ? sigp[k] : siga[k], 64 ); used += 64;
      d->pub_off = (uint32_t)used; memcpy( hb + used, pubp ? pubp[k] : puba[k], 32 ); used += 32;
      if( shared_msg ) { d->msg_off = (uint32_t)shared_off; d->msg_sz = (uint32_t)shared_sz; }
      else {
        d->msg_off = (uint32_t)used; d->msg_sz = (uint32_t)msz;
        if( msz ) memcpy( hb + used, msg[k], msz );
        used += msz;
      }
      cnt++;
    }
    unsigned long ticket = 0;
    int r = fd_ed25519_gpu_try_submit( g, cnt, hb, used, dd, &ticket );
    if( r != 1 ) { if( !r ) fd_ed25519_gpu_unstage( g, hb ); return r < 0 ? r : FD_ED25519_ERR_GPU; }   /* a failed submit released it */
    r = fd_ed25519_gpu_poll( g, ticket, out + i, 1 );
    if( r != 1 ) {
      /* timed out or failed: nobody polls this ticket again, so its slot is
         orphaned (reclaimed once the batch drains), not lost to the engine */
      fd_abandon_ticket( g, ticket );
      return r < 0 ? r : FD_ED25519_ERR_GPU;
    }
    i += cnt;
  }
  return 0;
}

static int fd_first_err( unsigned long n, int const * out ) {
  for( unsigned long i=0; i<n; i++ ) if( out[i] ) return out[i];
  return 0;
}

extern "C" int fd_ed25519_verify_batch( unsigned long n, uint8_t const * const * msg, unsigned long const * msg_sz,
                                        uint8_t const * const * sig, uint8_t const * const * pub, int * out_err ) {
  if( !n ) return 0;
  if( !msg || !msg_sz || !sig || !pub || !out_err ) return FD_ED25519_ERR_ARG;
  for( unsigned long i=0; i<n; i++ ) if( !sig[i] || !pub[i] || (msg_sz[i] && !msg[i]) ) return FD_ED25519_ERR_ARG;
  int err = fd_run_ptr_batch( fd_default_engine(), n, msg, msg_sz, NULL, 0, sig, NULL, pub, NULL, out_err );
  if( err ) return err;
  return fd_first_err( n, out_err );
}

extern "C" int fd_ed25519_gpu_verify_ptrs( fd_ed25519_gpu_t * g, unsigned long n, uint8_t const * const * msg,
                                           unsigned long const * msg_sz, uint8_t const * const * sig,
                                           uint8_t const * const * pub, int * out ) {
  if( !g ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  if( !msg || !msg_sz || !sig || !pub || !out ) return FD_ED25519_ERR_ARG;
  for( unsigned long i=0; i<n; i++ ) if( !sig[i] || !pub[i] || (msg_sz[i] && !msg[i]) ) return FD_ED25519_ERR_ARG;
  int err = fd_run_ptr_batch( g, n, msg, msg_sz, NULL, 0, sig, NULL, pub, NULL, out );
  if( err ) return err;
  return fd_first_err( n, out );
}

extern "C" int fd_ed25519_verify_batch_single_msg( uint8_t const * msg, unsigned long msg_sz, uint8_t const (*sig)[64],
                                                   uint8_t const (*pub)[32], unsigned long n, int * out_err_opt ) {
  if( !n ) return 0;
  if( !sig || !pub || (msg_sz && !msg) ) return FD_ED25519_ERR_ARG;
  int * out = out_err_opt;
  int * tmp = NULL;
  if( !out ) { tmp = (int *)malloc( n * sizeof(int) ); if( !tmp ) return FD_ED25519_ERR_GPU; out = tmp; }
  static uint8_t const empty[1] = { 0 };
  int err = fd_run_ptr_batch( fd_default_engine(), n, NULL, NULL, msg_sz ? msg : empty, msg_sz, NULL, sig, NULL, pub, out );
  int r = err ? err : fd_first_err( n, out );
  free( tmp );
  return r;
}

/* fd_ed25519_verify (fd_ed25519.h:96-101): one signature per call.  Calls
   from several threads coalesce into shared batches (group commit): a call
   joins the queue; if fewer than fd_vq_leaders() batches are running it
   leads -- it takes every queued call (up to FD_VQ_MAX) as one batch on
   the process-default engine, hands each call its own code and wakes the
   rest; a call arriving while fd_vq_leaders() batches run waits and rides
   the next one.  Leaders' batches run side by side on the engine's ring
   slots (fd_run_ptr_batch holds the engine lock only to take a slot,
   enqueue and collect), so a call that arrives while another batch is in
   flight does not wait a whole extra round trip behind it: with 4
   concurrent callers and one leader at a time, every call waited for the
   batch ahead of it (p50 0.95 ms for a 0.46 ms round trip,
   profiles/r03_per_signature_threads.jsonl). */
#define FD_VQ_MAX     4096UL
struct fd_vreq { uint8_t const * m; unsigned long sz; uint8_t const * s; uint8_t const * p; int out; int done; };
static std::mutex              fd_vq_lock;
static std::condition_variable fd_vq_cv;
static std::deque<fd_vreq *>   fd_vq;
static int                     fd_vq_running = 0;

static void fd_vq_run( std::vector<fd_vreq *> const & b, std::vector<int> & code ) {
  unsigned long n = b.size();
  std::vector<uint8_t const *> m, s, p; std::vector<unsigned long> sz; std::vector<unsigned long> idx;
  fd_ed25519_gpu_t * g = fd_default_engine();
  code.assign( n, FD_ED25519_ERR_GPU );
  for( unsigned long k=0; k<n; k++ ) {
    fd_vreq const * r = b[k];
    if( !r->s || !r->p || (r->sz && !r->m) ) { code[k] = FD_ED25519_ERR_ARG; continue; }
    m.push_back( r->m ); s.push_back( r->s ); p.push_back( r->p ); sz.push_back( r->sz ); idx.push_back( k );
  }
  if( idx.empty() ) return;
  std::vector<int> out( idx.size() );
  int err = fd_run_ptr_batch( g, idx.size(), m.data(), sz.data(), NULL, 0, s.data(), NULL, p.data(), NULL, out.data() );
  for( unsigned long j=0; j<idx.size(); j++ ) code[idx[j]] = err ? err : out[j];
}

extern "C" int fd_ed25519_verify( void const * msg, unsigned long sz, void const * sig, void const * public_key, void * sha ) {
  (void)sha;
  fd_vreq me = { (uint8_t const *)msg, sz, (uint8_t const *)sig, (uint8_t const *)public_key, 0, 0 };
  std::unique_lock<std::mutex> lk( fd_vq_lock );
  fd_vq.push_back( &me );
  while( !me.done ) {
    /* lead only while this call is still queued (a leader may have taken it) */
    if( fd_vq_running >= fd_vq_leaders() || fd_vq.empty() ) { fd_vq_cv.wait( lk ); continue; }
    fd_vq_running++;
    std::vector<fd_vreq *> b;
    while( !fd_vq.empty() && b.size() < FD_VQ_MAX ) { b.push_back( fd_vq.front() ); fd_vq.pop_front(); }
    lk.unlock();
    std::vector<int> code;
    fd_vq_run( b, code );
    lk.lock();
    for( unsigned long k=0; k<b.size(); k++ ) { b[k]->out = code[k]; b[k]->done = 1; }
    fd_vq_running--;
    fd_vq_cv.notify_all();
  }
  return me.out;
}

extern "C" char const * fd_ed25519_strerror( int err ) {
  switch( err ) {
  case FD_ED25519_SUCCESS:    return "success";
  case FD_ED25519_ERR_SIG:    return "bad signature";
  case FD_ED25519_ERR_PUBKEY: return "bad public key";
  case FD_ED25519_ERR_MSG:    return "bad message";
  case FD_ED25519_ERR_ARG:    return "bad argument";
  case FD_ED25519_ERR_GPU:    return "gpu failure";
  case FD_ED25519_ERR_TXN:    return "malformed transaction";
  default: break;
  }
  return "unknown";
}

/* ------------------------------------------------------------------ */
/* Batch signing and key derivation (include/fd_ed25519_gpu_sign.h). */

static int fd_sgn_batch_inv = FD_SGN_BATCH_INV;

extern "C" int fd_ed25519_gpu_sign_set_batch_inv( int on ) {
  return __atomic_exchange_n( &fd_sgn_batch_inv, on ? 1 : 0, __ATOMIC_RELAXED );
}

/* per signature of a slot's working set (its table scratch, 1536 B per
   signature): R || S, the key, the status */
#define FD_SGN_OUT_PER_SIG 100UL

/* Run one staged signing / derivation batch on a slot and collect its
   100 n (sign) or 32 n (derive) result bytes in sl->h_sgn.  in_sz bytes of
   sl->h_blob go to the device in one copy; whatever the outcome, the first
   clear_sz bytes (where seeds may lie) of the device blob are cleared by the
   slot's stream behind the kernel and those of the pinned blob by the
   host.  Caller holds g->lock and has set the device. */
static int fd_sgn_run( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long n, unsigned long in_sz, unsigned long clear_sz,
                       unsigned long blob_sz, unsigned long doff, int sign ) {
  hipError_t e;
  hipStream_t st = sl->stream;
  int err = 0;
  uint8_t * d_res = (uint8_t *)sl->work.tab;
  unsigned long res_sz = ( sign ? FD_SGN_OUT_PER_SIG : 32UL ) * n;
  int binv = __atomic_load_n( &fd_sgn_batch_inv, __ATOMIC_RELAXED );
  if( !sl->h_sgn && (e = hipHostMalloc( (void **)&sl->h_sgn, g->max_sigs * FD_SGN_OUT_PER_SIG, hipHostMallocDefault )) != hipSuccess ) {
    sl->h_sgn = NULL;
    memset( sl->h_blob, 0, clear_sz );
    return fd_gpu_fail( "hipHostMalloc signing results", e );
  }
  if( (e = hipMemcpyAsync( sl->d_blob, sl->h_blob, in_sz, hipMemcpyHostToDevice, st )) != hipSuccess ) err = fd_gpu_fail( "H2D signing batch", e );
  else if( (e = sign ? fd_ed25519_gpu_launch_sign( n, sl->d_blob, blob_sz, (fd_ed25519_gpu_sign_desc_t const *)(sl->d_blob + doff),
                                                   d_res, d_res + 64UL*n, (int32_t *)(d_res + 96UL*n), binv, st )
                     : fd_ed25519_gpu_launch_public( n, sl->d_blob, d_res, 1, binv, st )) != hipSuccess ) err = fd_gpu_fail( "launch sign", e );
  else if( (e = hipMemcpyAsync( sl->h_sgn, d_res, res_sz, hipMemcpyDeviceToHost, st )) != hipSuccess ) err = fd_gpu_fail( "D2H signatures", e );
  else if( (e = hipMemsetAsync( sl->d_blob, 0, clear_sz, st )) != hipSuccess ) err = fd_gpu_fail( "clear seeds", e );
  else if( (e = hipEventRecord( sl->done, st )) != hipSuccess ) err = fd_gpu_fail( "event", e );
  if( err ) {
    /* part of the batch may be queued: the clear goes behind it (best effort) */
    (void)hipMemsetAsync( sl->d_blob, 0, clear_sz, st );
    (void)hipGetLastError();
  }
  /* a slot orphaned here still has the clear on its stream ahead of its done event */
  err = fd_slot_settle( g, sl, st, err );
  memset( sl->h_blob, 0, clear_sz );
  return err;
}

extern "C" int fd_ed25519_gpu_sign_packed( fd_ed25519_gpu_t * g, unsigned long n, void const * blob, unsigned long blob_sz,
                                           fd_ed25519_gpu_sign_desc_t const * sdesc, void * sig_out, void * pub_out_opt, int * out ) {
  if( !g || n > g->max_sigs || blob_sz > g->max_blob || (n && (!sdesc || !sig_out || !out)) || (blob_sz && !blob) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, blob, &sl );
  if( err ) return err;
  unsigned long doff = fd_slot_stage( sl, blob, blob_sz, NULL, 0UL, sdesc, n * sizeof(fd_ed25519_gpu_sign_desc_t) );
  if( (err = fd_sgn_run( g, sl, n, doff + n * sizeof(fd_ed25519_gpu_sign_desc_t), blob_sz, blob_sz, doff, 1 )) ) return err;
  memcpy( sig_out, sl->h_sgn, 64UL*n );
  if( pub_out_opt ) memcpy( pub_out_opt, sl->h_sgn + 64UL*n, 32UL*n );
  memcpy( out, sl->h_sgn + 96UL*n, 4UL*n );
  sl->staged = 0;
  return 0;
}

extern "C" int fd_ed25519_gpu_public_packed( fd_ed25519_gpu_t * g, unsigned long n, void const * seeds, void * pub_out ) {
  if( !g || n > g->max_sigs || 32UL*n > g->blob_cap || (n && (!seeds || !pub_out)) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  memcpy( sl->h_blob, seeds, 32UL*n );
  if( (err = fd_sgn_run( g, sl, n, 32UL*n, 32UL*n, 0UL, 0UL, 0 )) ) return err;
  memcpy( pub_out, sl->h_sgn, 32UL*n );
  return 0;
}

extern "C" int fd_ed25519_gpu_sign_dev( fd_ed25519_gpu_t * g, unsigned long n, void const * d_blob, unsigned long blob_sz,
                                        fd_ed25519_gpu_sign_desc_t const * d_sdesc, void * d_sig_out, void * d_pub_out_opt,
                                        int * d_out, void * stream ) {
  if( !g || n > (1UL<<31) || (n && (!d_blob || !d_sdesc || !d_sig_out || !d_out))
      || ((uintptr_t)d_blob & 3UL) || ((uintptr_t)d_sig_out & 15UL) || ((uintptr_t)d_pub_out_opt & 15UL) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  hipStream_t st = stream ? (hipStream_t)stream : g->slot[0].stream;
  if( (e = fd_ed25519_gpu_launch_sign( n, (uint8_t const *)d_blob, blob_sz, d_sdesc, (uint8_t *)d_sig_out, (uint8_t *)d_pub_out_opt,
                                       (int32_t *)d_out, __atomic_load_n( &fd_sgn_batch_inv, __ATOMIC_RELAXED ), st )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_sign", e );
  return 0;
}

extern "C" int fd_ed25519_gpu_debug_sign_op( fd_ed25519_gpu_t * g, int op, unsigned long n, void const * in0, void const * in1,
                                             void const * in2, void * out ) {
  if( !g || op < 0 || op > 1 || n > (1UL<<20) || (n && (!in0 || !out || (op == 1 && (!in1 || !in2)))) ) return FD_ED25519_ERR_ARG;
  if( !n ) return 0;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  hipError_t e;
  hipStream_t st = sl->stream;
  unsigned long sz = 32UL * n;
  uint8_t * d = NULL;
  if( (e = hipMalloc( (void **)&d, 4UL * sz )) != hipSuccess ) return fd_gpu_fail( "debug_sign_op alloc", e );
  if( (e = hipMemcpyAsync( d, in0, sz, hipMemcpyHostToDevice, st )) != hipSuccess
   || ( op == 1 && ( (e = hipMemcpyAsync( d + sz, in1, sz, hipMemcpyHostToDevice, st )) != hipSuccess
                  || (e = hipMemcpyAsync( d + 2UL*sz, in2, sz, hipMemcpyHostToDevice, st )) != hipSuccess ) )
   || (e = ( op == 0 ? fd_ed25519_gpu_launch_public( n, d, d + 3UL*sz, 0, __atomic_load_n( &fd_sgn_batch_inv, __ATOMIC_RELAXED ), st )
                     : fd_ed25519_gpu_launch_debug_muladd( n, d, d + sz, d + 2UL*sz, d + 3UL*sz, st ) )) != hipSuccess
   || (e = hipMemcpyAsync( out, d + 3UL*sz, sz, hipMemcpyDeviceToHost, st )) != hipSuccess
   || (e = hipEventRecord( sl->done, st )) != hipSuccess ) err = fd_gpu_fail( "debug_sign_op", e );
  err = fd_slot_settle( g, sl, st, err );
  if( !fd_slot_in_flight( sl ) ) hipFree( d );
  return err;
}

/* fd_ed25519_sign_batch on an engine: consecutive elements are packed into
   a slot's pinned blob (seed, the key if given, the message) until the
   engine's max_sigs or max_blob is reached, signed as one packed batch and
   scattered; an element that cannot fit a blob on its own goes to the host
   routine. */
extern "C" int fd_ed25519_gpu_sign_batch( fd_ed25519_gpu_t * g, unsigned long n, unsigned char const * seed, unsigned char const * blob,
                                          uint64_t const * msg_off, uint32_t const * msg_sz, unsigned char * pub, unsigned char * sig,
                                          int derive ) {
  if( !g ) g = fd_default_engine();
  if( !g ) return FD_ED25519_ERR_GPU;
  if( n && (!seed || !msg_off || !msg_sz || !pub || !sig) ) return FD_ED25519_ERR_ARG;
  unsigned long max_sigs = g->max_sigs, max_blob = g->max_blob;
  unsigned long const fixed = derive ? 32UL : 64UL;
  std::vector<int> codes( max_sigs < n ? max_sigs : n );
  unsigned long i = 0;
  while( i < n ) {
    if( fixed + (unsigned long)msg_sz[i] > max_blob ) {
      if( derive ) fd_ed25519_public_from_private( pub + 32UL*i, seed + 32UL*i, NULL );
      fd_ed25519_sign( sig + 64UL*i, blob + msg_off[i], msg_sz[i], pub + 32UL*i, seed + 32UL*i, NULL );
      i++;
      continue;
    }
    void * sblob; fd_ed25519_gpu_desc_t * sdesc_;
    int err = fd_stage_wait( g, &sblob, &sdesc_ );
    if( err ) return err;
    fd_ed25519_gpu_sign_desc_t * sd = (fd_ed25519_gpu_sign_desc_t *)sdesc_;
    uint8_t * bl = (uint8_t *)sblob;
    unsigned long used = 0, cnt = 0;
    while( i + cnt < n && cnt < max_sigs && used + fixed + (unsigned long)msg_sz[i+cnt] <= max_blob ) {
      unsigned long j = i + cnt;
      memcpy( bl + used, seed + 32UL*j, 32UL );
      sd[cnt].seed_off = (uint32_t)used; used += 32UL;
      if( derive ) sd[cnt].pub_off = FD_ED25519_GPU_SIGN_DERIVE;
      else { memcpy( bl + used, pub + 32UL*j, 32UL ); sd[cnt].pub_off = (uint32_t)used; used += 32UL; }
      if( msg_sz[j] ) memcpy( bl + used, blob + msg_off[j], msg_sz[j] );
      sd[cnt].msg_off = (uint32_t)used; sd[cnt].msg_sz = msg_sz[j]; used += msg_sz[j];
      cnt++;
    }
    err = fd_ed25519_gpu_sign_packed( g, cnt, sblob, used, sd, sig + 64UL*i, derive ? pub + 32UL*i : NULL, codes.data() );
    if( err ) { memset( bl, 0, used ); fd_ed25519_gpu_unstage( g, sblob ); return err; }
    for( unsigned long k=0; k<cnt; k++ ) if( codes[k] ) return FD_ED25519_ERR_GPU;   /* descriptors built here are in bounds */
    i += cnt;
  }
  return 0;
}

extern "C" int fd_ed25519_sign_batch_gpu( unsigned long n, unsigned char const * seed, unsigned char const * blob, uint64_t const * msg_off,
                                          uint32_t const * msg_sz, unsigned char * pub, unsigned char * sig, int derive ) {
  return fd_ed25519_gpu_sign_batch( NULL, n, seed, blob, msg_off, msg_sz, pub, sig, derive );
}

/* ------------------------------------------------------------------ */
/* Whole transactions (include/fd_ed25519_gpu_txn.h). */

static inline unsigned long fd_al16( unsigned long x ) { return (x + 15UL) & ~15UL; }

/* the staging layout of the host-buffer calls (device and pinned alike):
   entries | results | n_sig | codes or descriptors (max_sigs) | fd_txn_t rows */
struct fd_txn_pk_off { unsigned long txn, res, nsig, sig, out; };
static fd_txn_pk_off fd_txn_pk_layout( unsigned long cap, unsigned long max_sigs ) {
  fd_txn_pk_off o;
  o.txn  = 0UL;
  o.res  = o.txn  + fd_al16( cap * sizeof(fd_ed25519_gpu_txn_t) );
  o.nsig = o.res  + fd_al16( cap * sizeof(fd_ed25519_gpu_txn_result_t) );
  o.sig  = o.nsig + 16UL;
  o.out  = o.sig  + fd_al16( max_sigs * sizeof(fd_ed25519_gpu_desc_t) );
  return o;
}

/* Scratch for n_txn transactions a call and out_sz bytes of fd_txn_t rows
   in the staging.  Growing waits for the device to go idle first (earlier
   calls may still use the old scratch).  Caller holds dev_lock and has set
   the device. */
static int fd_txn_ensure( fd_ed25519_gpu_t * g, unsigned long n_txn, unsigned long out_sz ) {
  hipError_t e;
  for( int b=0; b<2; b++ ) {
    fd_txn_set * ts = &g->txn_set[b];
    if( !ts->done  && (e = hipEventCreateWithFlags( &ts->done, hipEventDisableTiming )) != hipSuccess ) { ts->done = NULL; return fd_gpu_fail( "txn event", e ); }
    if( !ts->desc  && (e = hipMalloc( (void **)&ts->desc,  g->max_sigs * sizeof(fd_ed25519_gpu_desc_t) )) != hipSuccess ) { ts->desc = NULL; return fd_gpu_fail( "txn scratch", e ); }
    if( !ts->codes && (e = hipMalloc( (void **)&ts->codes, g->max_sigs * sizeof(int32_t) )) != hipSuccess ) { ts->codes = NULL; return fd_gpu_fail( "txn scratch", e ); }
  }
  for( int k=0; k<6; k++ )
    if( !g->txn_ev[k] && (e = hipEventCreate( &g->txn_ev[k] )) != hipSuccess ) { g->txn_ev[k] = NULL; return fd_gpu_fail( "txn event", e ); }
  unsigned long cap = g->txn_cap > n_txn ? g->txn_cap : n_txn;
  unsigned long need = fd_txn_pk_layout( cap, g->max_sigs ).out + out_sz;
  if( cap == g->txn_cap && need <= g->txn_pk_sz ) return 0;
  if( (e = hipDeviceSynchronize()) != hipSuccess ) return fd_gpu_fail( "txn scratch (idle)", e );
  if( cap != g->txn_cap ) {
    for( int b=0; b<2; b++ ) {
      fd_txn_set * ts = &g->txn_set[b];
      if( ts->meta ) hipFree( ts->meta );
      if( ts->part ) hipFree( ts->part );
      ts->meta = NULL; ts->part = NULL;
    }
    g->txn_cap = 0UL;
    for( int b=0; b<2; b++ ) {
      fd_txn_set * ts = &g->txn_set[b];
      if( (e = hipMalloc( (void **)&ts->meta, cap * sizeof(fd_txn_meta_t) )) != hipSuccess ) { ts->meta = NULL; return fd_gpu_fail( "txn scratch", e ); }
      if( (e = hipMalloc( (void **)&ts->part, fd_txn_part_cnt( cap ) * sizeof(uint32_t) )) != hipSuccess ) { ts->part = NULL; return fd_gpu_fail( "txn scratch", e ); }
    }
  }
  if( g->d_txn_pk ) hipFree( g->d_txn_pk );
  if( g->h_txn_pk ) hipHostFree( g->h_txn_pk );
  g->d_txn_pk = NULL; g->h_txn_pk = NULL; g->txn_pk_sz = 0UL;
  if( (e = hipMalloc( (void **)&g->d_txn_pk, need )) != hipSuccess ) { g->d_txn_pk = NULL; return fd_gpu_fail( "txn staging", e ); }
  if( (e = hipHostMalloc( (void **)&g->h_txn_pk, need, hipHostMallocDefault )) != hipSuccess ) { g->h_txn_pk = NULL; return fd_gpu_fail( "txn staging", e ); }
  g->txn_pk_sz = need;
  g->txn_cap   = cap;
  return 0;
}

/* The ring slots' own transaction scratch (descriptors, results between
   the kernels, the pinned results the host reads): every slot that has
   none yet gets it, so two batches in flight share nothing; timed: the
   engine's four timing events too.  Caller holds the ring lock and has set
   the device. */
static int fd_txn_ring_ensure( fd_ed25519_gpu_t * g, int timed ) {
  hipError_t e;
  for( int k=0; timed && k<4; k++ )
    if( !g->txn_ring_ev[k] && (e = hipEventCreate( &g->txn_ring_ev[k] )) != hipSuccess ) { g->txn_ring_ev[k] = NULL; return fd_gpu_fail( "txn event", e ); }
  for( int s=0; s<g->depth; s++ ) {
    fd_ed25519_gpu_slot * sl = &g->slot[s];
    if( sl->t_desc && sl->t_res && sl->h_res_dev ) continue;
    if( !sl->t_desc && (e = hipMalloc( (void **)&sl->t_desc, g->max_sigs * sizeof(fd_ed25519_gpu_desc_t) )) != hipSuccess ) { sl->t_desc = NULL; return fd_gpu_fail( "txn ring scratch", e ); }
    if( !sl->t_res  && (e = hipMalloc( (void **)&sl->t_res,  g->max_sigs * sizeof(fd_ed25519_gpu_txn_result_t) )) != hipSuccess ) { sl->t_res = NULL; return fd_gpu_fail( "txn ring scratch", e ); }
    if( !sl->h_res  && (e = hipHostMalloc( (void **)&sl->h_res, g->max_sigs * sizeof(fd_ed25519_gpu_txn_result_t),
                                           hipHostMallocMapped | hipHostMallocCoherent )) != hipSuccess ) { sl->h_res = NULL; return fd_gpu_fail( "txn ring results", e ); }
    if( (e = hipHostGetDevicePointer( (void **)&sl->h_res_dev, sl->h_res, 0 )) != hipSuccess ) { sl->h_res_dev = NULL; return fd_gpu_fail( "txn ring results (mapped)", e ); }
    g->txn_ring_allocs++;
  }
  return 0;
}

extern "C" int fd_ed25519_gpu_txns_reserve( fd_ed25519_gpu_t * g, unsigned long max_txn ) {
  if( !g || !max_txn || max_txn > FD_TXN_MAX ) return FD_ED25519_ERR_ARG;
  std::lock_guard<std::mutex> guard( g->dev_lock );
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  int err = fd_txn_ensure( g, max_txn, 0UL );
  if( err ) return err;
  /* the ring's slots too (dev_lock, then the ring lock, as
     fd_ed25519_gpu_verify_txns_packed orders them) */
  std::lock_guard<fd_ring_lock> rguard( g->lock );
  return fd_txn_ring_ensure( g, 0 );
}

static int fd_txn_args_ok( fd_ed25519_gpu_t const * g, unsigned long n_txn, void const * blob, unsigned long blob_sz, void const * txn,
                           void const * res, void const * txn_out, unsigned long stride ) {
  if( !g || n_txn > FD_TXN_MAX || blob_sz > 0xffffffffUL || (n_txn && (!txn || !res)) || (blob_sz && !blob) ) return 0;
  if( (uintptr_t)res & 7UL ) return 0;
  if( txn_out && ( stride < sizeof(fd_txn_t) || (stride & 1UL) || stride > 65534UL || ((uintptr_t)txn_out & 1UL) ) ) return 0;
  return 1;
}

/* The device-resident sequence on `st`, scratch set txn_seq mod 2: wait for
   the set, parse / scan / expand, the verify pipeline on sig_cap slots
   (fd_dev_launch orders it after the work on st and st after its codes),
   reduce.  verify == 0 (fd_ed25519_gpu_debug_txn_descs) stops after expand.
   ev: NULL or the six timing events.  *set_out: the set used.  Caller
   holds dev_lock and has called fd_txn_ensure. */
static int fd_txn_dev_run( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * d_blob, unsigned long blob_sz,
                           fd_ed25519_gpu_txn_t const * d_txn, unsigned long sig_cap, fd_ed25519_gpu_txn_result_t * d_res,
                           int * d_codes_opt, void * d_txn_out_opt, unsigned long stride, hipStream_t st, fd_knobs const & kn,
                           int verify, hipEvent_t const * ev, int * set_out ) {
  hipError_t e;
  int b = (int)(g->txn_seq & 1UL);
  fd_txn_set * ts = &g->txn_set[b];
  if( set_out ) *set_out = b;
  if( (e = hipStreamWaitEvent( st, ts->done, 0 )) != hipSuccess ) return fd_gpu_fail( "txn order", e );
  if( (e = fd_ed25519_gpu_launch_txn_front( n_txn, (uint8_t const *)d_blob, blob_sz, d_txn, sig_cap, d_res, (uint8_t *)d_txn_out_opt,
                                            d_txn_out_opt ? stride : 0UL, ts->meta, ts->part, ts->desc, st, ev )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_txn_front", e );
  if( verify && sig_cap ) {
    int32_t * codes = d_codes_opt ? (int32_t *)d_codes_opt : ts->codes;
    int err = fd_dev_launch( g, sig_cap, d_blob, blob_sz, ts->desc, codes, (void *)st, 0, kn );
    if( err ) return err;
    if( ev && (e = hipEventRecord( ev[4], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
    if( (e = fd_ed25519_gpu_launch_txn_reduce( n_txn, d_res, codes, st )) != hipSuccess )
      return fd_gpu_fail( "fd_ed25519_gpu_launch_txn_reduce", e );
    if( ev && (e = hipEventRecord( ev[5], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  } else if( ev ) {
    if( (e = hipEventRecord( ev[4], st )) != hipSuccess || (e = hipEventRecord( ev[5], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  }
  if( (e = hipEventRecord( ts->done, st )) != hipSuccess ) return fd_gpu_fail( "txn order", e );
  g->txn_seq++;
  return 0;
}

static int fd_txn_dev_call( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * d_blob, unsigned long blob_sz,
                            fd_ed25519_gpu_txn_t const * d_txn, unsigned long sig_cap, fd_ed25519_gpu_txn_result_t * d_res,
                            int * d_codes_opt, void * d_txn_out_opt, unsigned long stride, void * stream, float * kernel_ms ) {
  if( !fd_txn_args_ok( g, n_txn, d_blob, blob_sz, d_txn, d_res, d_txn_out_opt, stride ) || sig_cap > g->max_sigs || (n_txn && !d_blob) )
    return FD_ED25519_ERR_ARG;
  if( kernel_ms ) for( int k=0; k<4; k++ ) kernel_ms[k] = 0.f;
  if( !n_txn ) return 0;
  fd_knobs kn = fd_knobs_get( g );     /* before dev_lock: the engine's locks are never nested */
  std::lock_guard<std::mutex> guard( g->dev_lock );
  hipError_t e = hipSetDevice( g->device );
  if( e != hipSuccess ) return fd_gpu_fail( "hipSetDevice", e );
  int err = fd_txn_ensure( g, n_txn, 0UL );
  if( err ) return err;
  hipStream_t st = stream ? (hipStream_t)stream : g->slot[0].stream;
  err = fd_txn_dev_run( g, n_txn, d_blob, blob_sz, d_txn, sig_cap, d_res, d_codes_opt, d_txn_out_opt, stride, st, kn, 1,
                        kernel_ms ? g->txn_ev : NULL, NULL );
  if( err || !kernel_ms ) return err;
  if( (err = fd_event_wait( g->txn_ev[5], fd_timeout( g ) )) ) return err;
  for( int k=0; k<4; k++ )
    if( (e = hipEventElapsedTime( &kernel_ms[k], g->txn_ev[k == 3 ? 4 : k], g->txn_ev[k == 3 ? 5 : k+1] )) != hipSuccess )
      return fd_gpu_fail( "elapsed", e );
  return 0;
}

extern "C" int fd_ed25519_gpu_verify_txns_dev( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * d_blob, unsigned long blob_sz,
                                               fd_ed25519_gpu_txn_t const * d_txn, unsigned long sig_cap,
                                               fd_ed25519_gpu_txn_result_t * d_res, int * d_codes_opt, void * d_txn_out_opt,
                                               unsigned long txn_out_stride, void * stream ) {
  return fd_txn_dev_call( g, n_txn, d_blob, blob_sz, d_txn, sig_cap, d_res, d_codes_opt, d_txn_out_opt, txn_out_stride, stream, NULL );
}

extern "C" int fd_ed25519_gpu_verify_txns_dev_timed( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * d_blob, unsigned long blob_sz,
                                                     fd_ed25519_gpu_txn_t const * d_txn, unsigned long sig_cap,
                                                     fd_ed25519_gpu_txn_result_t * d_res, int * d_codes_opt, void * d_txn_out_opt,
                                                     unsigned long txn_out_stride, void * stream, float * kernel_ms ) {
  if( !kernel_ms ) return FD_ED25519_ERR_ARG;
  return fd_txn_dev_call( g, n_txn, d_blob, blob_sz, d_txn, sig_cap, d_res, d_codes_opt, d_txn_out_opt, txn_out_stride, stream, kernel_ms );
}

/* One launch of a host-buffer call on slot sl, whose device blob holds the
   batch: entries txn[0, nt) in, results, n_sig, codes (verify) or
   descriptors, and fd_txn_t rows out, all through the staging; waits for
   it (fd_slot_settle: the blob copy fd_txn_blob_in queued is on the same
   stream).  Caller holds both engine locks. */
static int fd_txn_host_run( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long blob_sz, fd_ed25519_gpu_txn_t const * txn,
                            unsigned long nt, unsigned long cap, unsigned long stride, fd_knobs const & kn, int verify ) {
  hipError_t e;
  hipStream_t st = sl->stream;
  int err;
  do {
    if( (err = fd_txn_ensure( g, nt, nt * stride )) ) break;
    fd_txn_pk_off o = fd_txn_pk_layout( g->txn_cap, g->max_sigs );
    uint8_t * d = g->d_txn_pk, * h = g->h_txn_pk;
    memcpy( h + o.txn, txn, nt * sizeof(fd_ed25519_gpu_txn_t) );
    if( (e = hipMemcpyAsync( d + o.txn, h + o.txn, nt * sizeof(fd_ed25519_gpu_txn_t), hipMemcpyHostToDevice, st )) != hipSuccess ) {
      err = fd_gpu_fail( "H2D transactions", e ); break;
    }
    int b;
    if( (err = fd_txn_dev_run( g, nt, sl->d_blob, blob_sz, (fd_ed25519_gpu_txn_t const *)(d + o.txn), cap,
                               (fd_ed25519_gpu_txn_result_t *)(d + o.res), NULL, stride ? d + o.out : NULL, stride, st, kn, verify, NULL, &b )) )
      break;
    fd_txn_set * ts = &g->txn_set[b];
    unsigned long per = verify ? sizeof(int32_t) : sizeof(fd_ed25519_gpu_desc_t);
    if( (e = hipMemcpyAsync( h + o.res, d + o.res, nt * sizeof(fd_ed25519_gpu_txn_result_t), hipMemcpyDeviceToHost, st )) != hipSuccess
     || (e = hipMemcpyAsync( h + o.nsig, ts->part + fd_txn_part_cnt( nt ) - 1UL, sizeof(uint32_t), hipMemcpyDeviceToHost, st )) != hipSuccess
     || ( cap && (e = hipMemcpyAsync( h + o.sig, verify ? (void const *)ts->codes : (void const *)ts->desc, cap * per, hipMemcpyDeviceToHost, st )) != hipSuccess )
     || ( stride && (e = hipMemcpyAsync( h + o.out, d + o.out, nt * stride, hipMemcpyDeviceToHost, st )) != hipSuccess )
     || (e = hipEventRecord( sl->done, st )) != hipSuccess ) err = fd_gpu_fail( "D2H transactions", e );
  } while(0);
  if( err ) (void)hipGetLastError();
  return fd_slot_settle( g, sl, st, err );
}

/* the batch's bytes into slot sl's device blob (with the pad the kernels
   may read past blob_sz); the caller settles a failure */
static int fd_txn_blob_in( fd_ed25519_gpu_slot * sl, void const * blob, unsigned long blob_sz ) {
  if( blob_sz ) memcpy( sl->h_blob, blob, blob_sz );
  memset( sl->h_blob + blob_sz, 0, FD_BLOB_PAD );
  hipError_t e = hipMemcpyAsync( sl->d_blob, sl->h_blob, blob_sz + FD_BLOB_PAD, hipMemcpyHostToDevice, sl->stream );
  return e == hipSuccess ? 0 : fd_gpu_fail( "H2D transaction blob", e );
}

extern "C" int fd_ed25519_gpu_verify_txns_packed( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                                                  fd_ed25519_gpu_txn_t const * txn, fd_ed25519_gpu_txn_result_t * res, int * codes_opt,
                                                  void * txn_out_opt, unsigned long txn_out_stride ) {
  if( !g || blob_sz > g->max_blob ) return FD_ED25519_ERR_ARG;
  /* results are staged, so the caller's res needs no alignment */
  if( !fd_txn_args_ok( g, 0UL, blob, blob_sz, txn, NULL, txn_out_opt, txn_out_stride ) || (n_txn && (!txn || !res)) )
    return FD_ED25519_ERR_ARG;
  if( !n_txn ) return 0;
  unsigned long stride = txn_out_opt ? txn_out_stride : 0UL;
  fd_knobs kn = fd_knobs_get( g );
  /* both engine locks, dev_lock first, as fd_ed25519_gpu_debug_k */
  std::lock_guard<std::mutex> dguard( g->dev_lock );
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  if( (err = fd_txn_blob_in( sl, blob, blob_sz )) ) return fd_slot_settle( g, sl, sl->stream, err );
  /* nothing is written on failure: everything lands in these first */
  std::vector<fd_ed25519_gpu_txn_result_t> hres( n_txn );
  std::vector<int32_t> hcodes;
  std::vector<uint8_t> hout( stride ? n_txn * stride : 0UL );
  unsigned long sig_total = 0UL, i = 0UL;
  while( i < n_txn ) {
    /* the longest run of transactions claiming at most max_sigs signatures */
    unsigned long j = i, claimed = 0UL;
    while( j < n_txn && j - i < FD_TXN_MAX ) {
      unsigned long c = fd_txn_claim( (uint8_t const *)blob, blob_sz, &txn[j] );
      if( j > i && claimed + c > g->max_sigs ) break;
      claimed += c; j++;
    }
    unsigned long nt = j - i, cap = claimed < g->max_sigs ? claimed : g->max_sigs;
    if( (err = fd_txn_host_run( g, sl, blob_sz, txn + i, nt, cap, stride, kn, 1 )) ) return err;
    fd_txn_pk_off o = fd_txn_pk_layout( g->txn_cap, g->max_sigs );
    uint8_t const * h = g->h_txn_pk;
    unsigned long n_sig = *(uint32_t const *)(h + o.nsig);
    if( n_sig > cap ) { snprintf( fd_gpu_err, sizeof(fd_gpu_err), "verify_txns: %lu slots taken of %lu", n_sig, cap ); return FD_ED25519_ERR_GPU; }
    memcpy( &hres[i], h + o.res, nt * sizeof(fd_ed25519_gpu_txn_result_t) );
    for( unsigned long t=i; t<j; t++ ) hres[t].sig_base += (uint32_t)sig_total;
    if( codes_opt ) hcodes.insert( hcodes.end(), (int32_t const *)(h + o.sig), (int32_t const *)(h + o.sig) + n_sig );
    if( stride ) memcpy( &hout[i * stride], h + o.out, nt * stride );
    sig_total += n_sig;
    i = j;
  }
  memcpy( res, hres.data(), n_txn * sizeof(fd_ed25519_gpu_txn_result_t) );
  if( codes_opt && sig_total ) memcpy( codes_opt, hcodes.data(), sig_total * sizeof(int32_t) );
  if( stride )
    for( unsigned long t=0; t<n_txn; t++ ) {
      unsigned long fp = hres[t].footprint;
      if( fp && fp <= stride ) memcpy( (uint8_t *)txn_out_opt + t * stride, &hout[t * stride], fp );
    }
  return 0;
}

extern "C" int fd_ed25519_gpu_debug_txn_descs( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                                               fd_ed25519_gpu_txn_t const * txn, unsigned long sig_cap, fd_ed25519_gpu_desc_t * desc_out,
                                               unsigned long * n_sig_out, fd_ed25519_gpu_txn_result_t * res_opt ) {
  if( !g || !n_txn || n_txn > FD_TXN_MAX || blob_sz > g->max_blob || sig_cap > g->max_sigs || !txn || !n_sig_out || (sig_cap && !desc_out)
      || (blob_sz && !blob) ) return FD_ED25519_ERR_ARG;
  fd_knobs kn = fd_knobs_get( g );
  std::lock_guard<std::mutex> dguard( g->dev_lock );
  std::lock_guard<fd_ring_lock> guard( g->lock );
  fd_ed25519_gpu_slot * sl;
  int err = fd_slot_take( g, NULL, &sl );
  if( err ) return err;
  if( (err = fd_txn_blob_in( sl, blob, blob_sz )) ) return fd_slot_settle( g, sl, sl->stream, err );
  if( (err = fd_txn_host_run( g, sl, blob_sz, txn, n_txn, sig_cap, 0UL, kn, 0 )) ) return err;
  fd_txn_pk_off o = fd_txn_pk_layout( g->txn_cap, g->max_sigs );
  uint8_t const * h = g->h_txn_pk;
  *n_sig_out = *(uint32_t const *)(h + o.nsig);
  if( sig_cap ) memcpy( desc_out, h + o.sig, sig_cap * sizeof(fd_ed25519_gpu_desc_t) );
  if( res_opt ) memcpy( res_opt, h + o.res, n_txn * sizeof(fd_ed25519_gpu_txn_result_t) );
  return 0;
}

/* ------------------------------------------------------------------ */
/* Transactions through the ring (fd_ed25519_gpu_submit_txns). */

/* A transaction batch: its tail, the entries and the claim prefix, is
   built where fd_ring_place says (behind the staged blob, or beside a
   registered one in the slot's mapped descriptor buffer).  Then
   fd_k_txn_ring_front, the ring's verify launch with the slot's
   transaction descriptors, and fd_k_txn_ring_reduce, which leaves the
   results in the slot's mapped pinned h_res (final only then: no poll
   takes the codes early).  ev: NULL, or four events around the front
   kernel and the reduce. */
static int fd_txn_slot_enqueue_( fd_ed25519_gpu_t * g, fd_ed25519_gpu_slot * sl, unsigned long n_txn, void const * blob,
                                 unsigned long blob_sz, fd_ed25519_gpu_txn_t const * txn, hipStream_t * used, hipEvent_t const * ev ) {
  unsigned long txn_sz = n_txn * sizeof(fd_ed25519_gpu_txn_t);
  /* <= 16 n_txn <= the descriptors' room */
  fd_ring_src p = fd_ring_place( g, sl, blob, blob_sz, NULL, 0UL, NULL, txn_sz + ( n_txn + 1UL ) * sizeof(uint32_t) );
  memcpy( p.tail, txn, txn_sz );
  /* the slot layout, read from the caller's bytes: a blob that was just
     staged is in the cache from the copy, one read in place from the pass
     fd_txn_try_submit made before it took the lock.  Should the bytes
     change between this and the DMA, the front kernel refuses whatever
     parses to another count than it claims here */
  unsigned long n_sig = fd_ed25519_gpu_txn_claims( blob, blob_sz, txn, n_txn, (uint32_t *)( p.tail + txn_sz ) );
  if( n_sig > g->max_sigs ) return FD_ED25519_ERR_ARG;   /* nothing queued */
  hipStream_t st = *used = fd_ring_stream( g, sl, n_sig );
  hipError_t e;
  uint8_t const * dt = (uint8_t const *)fd_ring_h2d( sl, p, st );
  if( !dt ) return FD_ED25519_ERR_GPU;
  /* nothing to verify: the front kernel's results are final, straight to
     the pinned results */
  if( ev && (e = hipEventRecord( ev[0], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  if( (e = fd_ed25519_gpu_launch_txn_ring_front( n_txn, n_sig, sl->d_blob, blob_sz, (fd_ed25519_gpu_txn_t const *)dt,
                                                 (uint32_t const *)( dt + txn_sz ), n_sig ? sl->t_res : sl->h_res_dev, sl->t_desc,
                                                 st )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_txn_ring_front", e );
  if( ev && (e = hipEventRecord( ev[1], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  int32_t * codes = fd_ring_verify( g, sl, n_sig, blob_sz, sl->t_desc, st, 0 );   /* n_sig 0: launches nothing */
  if( !codes ) return FD_ED25519_ERR_GPU;
  if( ev && (e = hipEventRecord( ev[2], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  if( n_sig && (e = fd_ed25519_gpu_launch_txn_ring_reduce( n_txn, n_sig, sl->t_res, codes, sl->h_res_dev, st )) != hipSuccess )
    return fd_gpu_fail( "fd_ed25519_gpu_launch_txn_ring_reduce", e );
  if( ev && (e = hipEventRecord( ev[3], st )) != hipSuccess ) return fd_gpu_fail( "txn event", e );
  if( fd_ring_finish( sl, n_sig, codes, st ) ) return FD_ED25519_ERR_GPU;
  sl->n = n_sig; sl->n_txn = n_txn;
  return 0;
}

static int fd_txn_try_submit( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                              fd_ed25519_gpu_txn_t const * txn, unsigned long * ticket, int timed ) {
  if( !g || !ticket || !txn || !n_txn || n_txn > g->max_sigs || n_txn > FD_TXN_MAX || blob_sz > g->max_blob || (blob_sz && !blob) )
    return FD_ED25519_ERR_ARG;
  /* A blob that will be read where it lies (a registered region, a slot's
     staged buffer) is walked once before the ring lock is taken for good:
     this pass takes the cache misses of a cold blob (one line per
     transaction, ~17 ns each) and refuses a batch that claims too much
     before any slot is looked at; the pass that writes the prefix, under
     the lock, then finds those lines warm (~2 ns each).  A blob that will
     be copied into a slot is walked after the copy, which warms it. */
  int in_place = 0;
  if( blob_sz ) {
    std::lock_guard<fd_ring_lock> guard( g->lock );
    in_place = fd_registered( g, blob, blob_sz ) || fd_slot_by_blob( g, blob );
  }
  if( in_place ) {
    unsigned long n_sig = 0UL;
    for( unsigned long t=0UL; t<n_txn; t++ ) {
      n_sig += fd_txn_claim( (uint8_t const *)blob, blob_sz, txn + t );
      if( n_sig > g->max_sigs ) return FD_ED25519_ERR_ARG;
    }
  }
  /* the scratch is allocated only if fd_ed25519_gpu_txns_reserve has not */
  return fd_ring_submit( g, blob, ticket, [&]{ return fd_txn_ring_ensure( g, timed ); }, [&]( fd_ed25519_gpu_slot * sl, hipStream_t * st ) {
    return fd_txn_slot_enqueue_( g, sl, n_txn, blob, blob_sz, txn, st, timed ? g->txn_ring_ev : NULL );
  } );
}

extern "C" int fd_ed25519_gpu_try_submit_txns( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                                               fd_ed25519_gpu_txn_t const * txn, unsigned long * ticket ) {
  return fd_txn_try_submit( g, n_txn, blob, blob_sz, txn, ticket, 0 );
}

extern "C" int fd_ed25519_gpu_submit_txns( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                                           fd_ed25519_gpu_txn_t const * txn, unsigned long * ticket ) {
  return fd_submit_code( fd_txn_try_submit( g, n_txn, blob, blob_sz, txn, ticket, 0 ) );
}

extern "C" int fd_ed25519_gpu_poll_txns( fd_ed25519_gpu_t * g, unsigned long ticket, fd_ed25519_gpu_txn_result_t * res, int * codes_opt,
                                         int block ) {
  if( !g || !ticket || !res ) return FD_ED25519_ERR_ARG;
  return fd_ring_poll( g, ticket, block, codes_opt, res );
}

extern "C" unsigned long fd_ed25519_gpu_txn_ring_allocs( fd_ed25519_gpu_t * g ) {
  if( !g ) return 0UL;
  std::lock_guard<fd_ring_lock> guard( g->lock );
  return g->txn_ring_allocs;
}

extern "C" int fd_ed25519_gpu_txn_ring_timed( fd_ed25519_gpu_t * g, unsigned long n_txn, void const * blob, unsigned long blob_sz,
                                              fd_ed25519_gpu_txn_t const * txn, fd_ed25519_gpu_txn_result_t * res, float * kernel_ms ) {
  if( !kernel_ms || !res ) return FD_ED25519_ERR_ARG;
  unsigned long ticket = 0UL;
  int r = fd_submit_code( fd_txn_try_submit( g, n_txn, blob, blob_sz, txn, &ticket, 1 ) );
  if( r ) return r;
  if( (r = fd_ed25519_gpu_poll_txns( g, ticket, res, NULL, 1 )) != 1 ) {
    if( r < 0 ) fd_abandon_ticket( g, ticket );
    return r < 0 ? r : FD_ED25519_ERR_GPU;
  }
  /* the events are the engine's: two timed calls at once would share them
     (a diagnostic, as fd_ed25519_gpu_verify_txns_dev_timed) */
  hipError_t e;
  if( (e = hipEventElapsedTime( &kernel_ms[0], g->txn_ring_ev[0], g->txn_ring_ev[1] )) != hipSuccess
   || (e = hipEventElapsedTime( &kernel_ms[1], g->txn_ring_ev[2], g->txn_ring_ev[3] )) != hipSuccess ) return fd_gpu_fail( "elapsed", e );
  return 0;
}
