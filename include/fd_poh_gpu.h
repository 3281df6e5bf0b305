#ifndef HEADER_fd_poh_gpu_h
#define HEADER_fd_poh_gpu_h

/* fd_poh_gpu.h -- Proof-of-History verification: batched SHA-256 chains.

   The reference has the scalar loop only (src/ballet/poh/fd_poh.c:3-24):
   fd_poh_append is n times state <- SHA-256( state ), fd_poh_mixin is
   state <- SHA-256( state || mixin ).  A ledger entry's hash is what these
   make of the previous entry's hash, so once every entry starts from the
   hash its predecessor CLAIMS, the entries of a batch are independent:
   one lane per entry, no exchange (fd_k_poh).

   An entry is

     state = start; fd_poh_append( state, n );
     if( flags & FD_POH_GPU_MIXIN ) fd_poh_mixin( state, mixin );
     code = state == expect ? 0 : FD_POH_ERR_HASH

   exactly the reference's two functions.  Solana's entry rule ("an entry
   of num_hashes with transactions is num_hashes - 1 appends, then the
   mixin") is the caller's: INTEGRATION.md shows the mapping.

   A chain is serial, so one entry runs at one lane's rate (a few
   microseconds per hash): the device path is for replay and catch-up
   batches of tens of thousands of entries and more.  Single calls and a
   single live slot stay on the host (fd_poh_append, fd_poh_mixin,
   fd_poh_verify_batch). */

#include "fd_ed25519_gpu.h"
#include "fd_bmtree_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FD_POH_GPU_MIXIN   (1U)
#define FD_POH_ERR_HASH    (-1)      /* chain does not reach expect */

/* launches one call may queue (n_max / C rounded up); more: FD_ED25519_ERR_ARG */
#define FD_POH_GPU_LAUNCH_MAX (1UL<<20)
/* hashes one lane runs per launch unless fd_poh_gpu_debug_set_chunk says
   otherwise: a 12,500-hash tick is never split */
#define FD_POH_GPU_CHUNK_DEFAULT (16384UL)

typedef struct {                     /* 112 bytes, 8-byte aligned */
  uint8_t  start[32];
  uint8_t  mixin[32];                /* read only with FD_POH_GPU_MIXIN */
  uint8_t  expect[32];
  uint64_t n;                        /* fd_poh_append count */
  uint32_t flags;
  uint32_t _pad;                     /* zero */
} fd_poh_gpu_entry_t;

/* The reference's state and its two functions (src/ballet/poh/fd_poh.h),
   on the host: n recursive hashes; one 32-byte mixin.  Both return poh.
   Where the reference's own header is in the translation unit its
   declarations stand. */
#ifndef HEADER_fd_src_ballet_poh_fd_poh_h
struct __attribute__((aligned(32))) fd_poh_state { uint8_t state[32]; };
typedef struct fd_poh_state fd_poh_state_t;

fd_poh_state_t * fd_poh_append( fd_poh_state_t * poh, unsigned long n );
fd_poh_state_t * fd_poh_mixin ( fd_poh_state_t * poh, uint8_t const * mixin );
#endif

/* The entry semantics above on nthreads host threads (1..256; entries are
   dealt to the threads in small runs as they finish, so a ragged batch
   balances).  out[i] is 0, FD_POH_ERR_HASH or FD_ED25519_ERR_ARG (unknown
   flag bits, nonzero _pad, n > n_max: never hashed, state_out 32 zero
   bytes); state_out_opt (NULL, or 32 n bytes) gets each entry's final
   state whether or not it matches.  Returns 0 or FD_ED25519_ERR_ARG (NULL
   array, thread count). */
int
fd_poh_verify_batch( unsigned long              n,
                     fd_poh_gpu_entry_t const * entries,
                     unsigned long              n_max,
                     int *                      out,
                     void *                     state_out_opt,
                     int                        nthreads );

/* The same on the device: synchronous, host buffers, any n (up to 2^31-1
   entries).  The lanes are ordered by n descending, so the waves are
   uniform, the long chains start first and launch j (of ceil( max n / C ),
   at least one) covers only the lanes with n > j C.  Scratch is the
   call's own, grows on demand and is not sized by the engine's max_sigs.
   Every wait is bounded by the engine's timeout.  gpu may be NULL: the
   process-default engine.  Returns 0, FD_ED25519_ERR_ARG (NULL array, n
   or the launch count out of range) or FD_ED25519_ERR_GPU (device error,
   timeout); on FD_ED25519_ERR_GPU nothing is written. */
int
fd_poh_gpu_verify_packed( fd_ed25519_gpu_t *         gpu,
                          unsigned long              n,
                          fd_poh_gpu_entry_t const * entries,
                          unsigned long              n_max,
                          int *                      out,
                          void *                     state_out_opt );

/* Device-resident: d_entries, d_out, d_state_out_opt (NULL, or 32 n bytes,
   16-byte aligned) and d_work (fd_poh_gpu_work_sz( n ) bytes, 16-byte
   aligned, the call's for as long as it runs) are device pointers.  Lanes run in the caller's
   order.  ceil( n_max / C ) launches (at least one) are queued on `stream`
   (a hipStream_t; NULL: the engine's PoH stream), in order with the work
   before and after them there; no host synchronisation.  An entry is done
   at the launch its count runs out; from then on its lane costs one load
   per launch.  Returns 0, FD_ED25519_ERR_ARG or FD_ED25519_ERR_GPU (the
   launch failed). */
int
fd_poh_gpu_verify_dev( fd_ed25519_gpu_t *         gpu,
                       unsigned long              n,
                       fd_poh_gpu_entry_t const * d_entries,
                       unsigned long              n_max,
                       int *                      d_out,
                       void *                     d_state_out_opt,
                       void *                     d_work,
                       void *                     stream );

unsigned long fd_poh_gpu_work_sz( unsigned long n );

/* Entries from leaves.  fd_poh_gpu_verify_packed with, per entry, the
   leaves of its mixin instead of the mixin: entry i has leaf_cnt[i] leaves
   (fd_bmtree_gpu.h: descriptors into blob, entry 0's first; typically the
   64-byte signatures of its transactions, in place in their payloads).

   An entry with leaf_cnt[i] == 0 is handled exactly as by
   fd_poh_gpu_verify_packed.  An entry with leaves must carry
   FD_POH_GPU_MIXIN; its mixin field is not read: the mixin is the bmtree32
   root of its leaves, computed on the device ahead of the chains.  Such an
   entry gets FD_ED25519_ERR_ARG and is never hashed if it lacks the flag or
   its tree is refused (leaf_cnt[i] > leaf_max, a leaf out of the blob or
   above FD_BMTREE_GPU_LEAF_SZ_MAX).  Returns as fd_poh_gpu_verify_packed;
   FD_ED25519_ERR_ARG also for a NULL leaf_cnt, leaf_max == 0,
   blob_sz >= 2^32 or more than FD_BMTREE_GPU_LEAVES_MAX leaves. */
int
fd_poh_gpu_verify_entries_packed( fd_ed25519_gpu_t *           gpu,
                                  unsigned long                n,
                                  fd_poh_gpu_entry_t const *   entries,
                                  unsigned long                n_max,
                                  int *                        out,
                                  void *                       state_out_opt,
                                  uint32_t const *             leaf_cnt,
                                  fd_bmtree_gpu_leaf_t const * leaves,
                                  void const *                 blob,
                                  unsigned long                blob_sz,
                                  unsigned long                leaf_max );

/* Device-resident: fd_poh_gpu_verify_dev's arguments, then the trees' as in
   fd_bmtree_gpu_roots_dev (d_first: the n + 1 exclusive prefix of the leaf
   counts) and d_tree_work (fd_poh_gpu_entries_work_sz( n, n_leaves ) bytes,
   16-byte aligned).  d_entries is written: the root goes into the mixin
   field of an entry with leaves (root_stride 112, offset 32), and _pad
   becomes nonzero where such an entry is refused, which is how the chain
   kernel comes to refuse it.  The tree launches (their number from
   min( leaf_max, n_leaves ) alone) are queued on `stream` ahead of the
   chain launches; no host synchronisation. */
int
fd_poh_gpu_verify_entries_dev( fd_ed25519_gpu_t *           gpu,
                               unsigned long                n,
                               fd_poh_gpu_entry_t *         d_entries,
                               unsigned long                n_max,
                               int *                        d_out,
                               void *                       d_state_out_opt,
                               void *                       d_work,
                               uint32_t const *             d_first,
                               unsigned long                n_leaves,
                               fd_bmtree_gpu_leaf_t const * d_leaves,
                               void const *                 d_blob,
                               unsigned long                blob_sz,
                               unsigned long                leaf_max,
                               void *                       d_tree_work,
                               void *                       stream );

unsigned long fd_poh_gpu_entries_work_sz( unsigned long n, unsigned long n_leaves );

/* Pure host code: start and expect of a run of n consecutive entries from
   the hash before the run and the hashes the entries claim: start[0] =
   seed, start[i] = hashes[i-1], expect[i] = hashes[i] (hashes: 32 n
   bytes).  n, mixin, flags and _pad are the caller's. */
void
fd_poh_gpu_chain( unsigned long        n,
                  uint8_t const *      seed,
                  uint8_t const *      hashes,
                  fd_poh_gpu_entry_t * entries );

/* Tests: hashes per lane per launch (1 .. 2^24; 0: the default), so tiny
   chains cross launch boundaries.  Returns 0 or FD_ED25519_ERR_ARG. */
int           fd_poh_gpu_debug_set_chunk( fd_ed25519_gpu_t * gpu, unsigned long C );
unsigned long fd_poh_gpu_chunk          ( fd_ed25519_gpu_t * gpu );

/* Experiments (tools/poh_bench.py): on = 0 makes fd_poh_gpu_verify_packed
   keep the caller's lane order, every launch covering every lane; the
   results are the same. */
int fd_poh_gpu_debug_set_sort( fd_ed25519_gpu_t * gpu, int on );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_poh_gpu_h */
