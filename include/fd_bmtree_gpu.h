#ifndef HEADER_fd_bmtree_gpu_h
#define HEADER_fd_bmtree_gpu_h

/* fd_bmtree_gpu.h -- binary Merkle trees over SHA-256 with 20- and 32-byte
   nodes (reference src/ballet/bmtree/fd_bmtree_tmpl.c): many roots per call
   on the device, and the reference's commit interface on the host.

     leaf   node: SHA-256( 0x00 || data )
     branch node: SHA-256( 0x01 || a[0,W) || b[0,W) ) truncated to W bytes

   A layer of c > 1 nodes has ceil( c / 2 ) parents; a node without a right
   sibling is merged with itself; a layer of one node is the root, so the
   root of a one-leaf tree is its leaf node.  Shreds use W = 20; a ledger
   entry's mixin is the W = 32 root over its transactions' signatures
   (fd_poh_gpu.h: fd_poh_gpu_verify_entries_packed / _dev).

   A tree's upper layers are short, so one tree keeps few lanes busy: the
   device path is for batches (one tree per entry or shred, hundreds of
   thousands per call) and for large trees.  Single small trees stay on
   the host (the commit interface below, fd_bmtree_roots_batch). */

#include "fd_ed25519_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's node and commit interface (src/ballet/bmtree/fd_bmtree.h),
   on the host.  Where the reference's own header is in the translation unit
   its declarations stand. */
#ifndef HEADER_fd_src_ballet_bmtree_fd_bmtree_h

#define FD_BMTREE20_HASH_SZ          (20UL)
#define FD_BMTREE20_COMMIT_ALIGN     (32UL)
#define FD_BMTREE20_COMMIT_FOOTPRINT (2048UL)
#define FD_BMTREE32_HASH_SZ          (32UL)
#define FD_BMTREE32_COMMIT_ALIGN     (32UL)
#define FD_BMTREE32_COMMIT_FOOTPRINT (2048UL)

/* hash[0,W) is the node; a 20-byte node leaves hash[20,32) undefined */
struct __attribute__((aligned(32))) fd_bmtree20_node { uint8_t hash[32]; };
struct __attribute__((aligned(32))) fd_bmtree32_node { uint8_t hash[32]; };
typedef struct fd_bmtree20_node fd_bmtree20_node_t;
typedef struct fd_bmtree32_node fd_bmtree32_node_t;

/* An incremental commitment: the leaves so far and, per layer, the last
   node that still waits for its right sibling.  O( log n ) space. */
struct fd_bmtree20_commit { unsigned long leaf_cnt; fd_bmtree20_node_t node_buf[63]; };
struct fd_bmtree32_commit { unsigned long leaf_cnt; fd_bmtree32_node_t node_buf[63]; };
typedef struct fd_bmtree20_commit fd_bmtree20_commit_t;
typedef struct fd_bmtree32_commit fd_bmtree32_commit_t;

/* node <- SHA-256( 0x00 || data[0,data_sz) ); returns node */
fd_bmtree20_node_t * fd_bmtree20_hash_leaf( fd_bmtree20_node_t * node, void const * data, unsigned long data_sz );
fd_bmtree32_node_t * fd_bmtree32_hash_leaf( fd_bmtree32_node_t * node, void const * data, unsigned long data_sz );

unsigned long fd_bmtree20_commit_align    ( void );   /* 32 */
unsigned long fd_bmtree20_commit_footprint( void );   /* 2048 */
unsigned long fd_bmtree32_commit_align    ( void );
unsigned long fd_bmtree32_commit_footprint( void );

/* init: mem (aligned, footprint bytes) becomes an empty commitment.
   append: leaf_cnt more leaf nodes, in order.  fini: the root (W bytes
   inside the commitment, valid until it is initialised again); at least
   one leaf must have been appended. */
fd_bmtree20_commit_t * fd_bmtree20_commit_init    ( void * mem );
unsigned long          fd_bmtree20_commit_leaf_cnt( fd_bmtree20_commit_t const * bmt );
fd_bmtree20_commit_t * fd_bmtree20_commit_append  ( fd_bmtree20_commit_t * bmt, fd_bmtree20_node_t const * leaf, unsigned long leaf_cnt );
uint8_t *              fd_bmtree20_commit_fini    ( fd_bmtree20_commit_t * bmt );
fd_bmtree32_commit_t * fd_bmtree32_commit_init    ( void * mem );
unsigned long          fd_bmtree32_commit_leaf_cnt( fd_bmtree32_commit_t const * bmt );
fd_bmtree32_commit_t * fd_bmtree32_commit_append  ( fd_bmtree32_commit_t * bmt, fd_bmtree32_node_t const * leaf, unsigned long leaf_cnt );
uint8_t *              fd_bmtree32_commit_fini    ( fd_bmtree32_commit_t * bmt );

#endif /* HEADER_fd_src_ballet_bmtree_fd_bmtree_h */

/* A leaf: blob[off, off+sz).  A signature inside a transaction payload is a
   leaf in place. */
typedef struct { uint32_t off; uint32_t sz; } fd_bmtree_gpu_leaf_t;

/* descriptors point at ready W-byte nodes (sz == width): no leaf hash */
#define FD_BMTREE_GPU_LEAVES_ARE_NODES (1U)
/* a leaf is one lane's work and no launch may be unbounded */
#define FD_BMTREE_GPU_LEAF_SZ_MAX      (65535U)
/* leaves of one call */
#define FD_BMTREE_GPU_LEAVES_MAX       (0x7fffffffUL)

/* Many trees on nthreads host threads (1..256): the device call's semantics
   and the bench's yardstick.  Tree i has leaf_cnt[i] leaves, the
   descriptors of tree 0 first, then tree 1's, and so on.  roots_out is 32 n_trees
   bytes (a W = 20 root is followed by 12 zero bytes), codes_out n_trees
   ints.  codes_out[i] is 0, or FD_ED25519_ERR_ARG for a refused tree, which
   is never hashed and whose root is 32 zero bytes:
     leaf_cnt[i] == 0 or leaf_cnt[i] > leaf_max,
     a leaf with off + sz past blob_sz (or wrapping 32 bits),
     a leaf with sz > FD_BMTREE_GPU_LEAF_SZ_MAX,
     with FD_BMTREE_GPU_LEAVES_ARE_NODES a leaf with sz != width.
   A refused tree does not disturb its neighbours.  Returns 0 or
   FD_ED25519_ERR_ARG (NULL array, width not 20 or 32, unknown flags, the
   leaf counts summing past FD_BMTREE_GPU_LEAVES_MAX, thread count). */
int
fd_bmtree_roots_batch( unsigned                     width,
                       unsigned                     flags,
                       unsigned long                n_trees,
                       uint32_t const *             leaf_cnt,
                       fd_bmtree_gpu_leaf_t const * leaves,
                       void const *                 blob,
                       unsigned long                blob_sz,
                       unsigned long                leaf_max,
                       void *                       roots_out,
                       int *                        codes_out,
                       int                          nthreads );

/* The same on the device: synchronous, host buffers.  Scratch is the
   call's own, grows on demand and is not sized by the engine's max_sigs.
   Every wait is bounded by the engine's timeout.  gpu may be NULL: the
   process-default engine.  Returns 0, FD_ED25519_ERR_ARG (as above, and
   leaf_max == 0 or blob_sz >= 2^32) or FD_ED25519_ERR_GPU (no device,
   device error, timeout); on FD_ED25519_ERR_GPU nothing is written.
   There is no host fallback. */
int
fd_bmtree_gpu_roots_packed( fd_ed25519_gpu_t *           gpu,
                            unsigned                     width,
                            unsigned                     flags,
                            unsigned long                n_trees,
                            uint32_t const *             leaf_cnt,
                            fd_bmtree_gpu_leaf_t const * leaves,
                            void const *                 blob,
                            unsigned long                blob_sz,
                            unsigned long                leaf_max,
                            void *                       roots_out,
                            int *                        codes_out );

/* Device-resident.  d_first is the exclusive prefix of the leaf counts
   (n_trees + 1 words, d_first[0] = 0, d_first[n_trees] = n_leaves, not
   decreasing); d_leaves, d_blob, d_roots, d_codes and d_work
   (fd_bmtree_gpu_work_sz( n_trees, n_leaves ) bytes, 16-byte aligned, the
   call's for as long as it runs) are device pointers.  Tree i's root goes
   to d_roots + i root_stride as 32 bytes (W = 20: bytes 20..31 zero);
   d_roots and root_stride are multiples of 4, root_stride >= 32.  The
   launches are queued on `stream` (a hipStream_t; NULL: the engine's tree
   stream), in order with the work before and after them there; no host
   synchronisation.  Their number comes from min( leaf_max, n_leaves )
   alone: four to set up, one for the leaves, one per layer.  Returns 0,
   FD_ED25519_ERR_ARG or FD_ED25519_ERR_GPU (a launch failed). */
int
fd_bmtree_gpu_roots_dev( fd_ed25519_gpu_t *           gpu,
                         unsigned                     width,
                         unsigned                     flags,
                         unsigned long                n_trees,
                         uint32_t const *             d_first,
                         unsigned long                n_leaves,
                         fd_bmtree_gpu_leaf_t const * d_leaves,
                         void const *                 d_blob,
                         unsigned long                blob_sz,
                         unsigned long                leaf_max,
                         void *                       d_roots,
                         unsigned long                root_stride,
                         int *                        d_codes,
                         void *                       d_work,
                         void *                       stream );

unsigned long fd_bmtree_gpu_work_sz( unsigned long n_trees, unsigned long n_leaves );

/* tools/bmtree_bench.py: the 64-lane compression passes the merge launches
   of a call issue (waves times the blocks of one merge: 1 for W = 20, 2
   for W = 32), counted from the shapes alone. */
unsigned long
fd_bmtree_gpu_merge_passes( unsigned         width,
                            unsigned long    n_trees,
                            uint32_t const * leaf_cnt );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_bmtree_gpu_h */
