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

/* Inclusion proofs.  The reference has the commit interface only, so the
   proof format is this library's, pinned to the reference through the root
   every proof walks to.  A tree of c leaves has depth D = ceil( log2( c ) )
   (0 for c = 1); layer 0 is the leaf nodes and layer l+1 has
   ceil( c_l / 2 ) nodes.

     proof of leaf i: D nodes of W bytes, packed, level 0 first.  Node l is
       the layer-l node ( i >> l ) ^ 1, or, where that index is >= c_l (the
       node on the path has no right sibling and is merged with itself),
       the node i >> l itself.
     walk: node = leaf( data ) (or the ready node); for l = 0 .. depth-1,
       p = proof[l], node = ( idx >> l ) & 1 ? merge( p, node )
                                             : merge( node, p ).
       The result is the derived root.
     strict walk (leaf_cnt != 0): the walk of exactly that tree: depth ==
       ceil( log2( leaf_cnt ) ), idx < leaf_cnt, and at a level where
       ( idx >> l ) ^ 1 >= c_l the proof node is not read and the node is
       merged with itself, so a prover cannot choose that sibling. */

/* the walk does not reach the expected root */
#define FD_BMTREE_ERR_PROOF (-1)

/* Emit.  The roots calls, and every leaf's proof: leaf k of the call, in
   descriptor order, gets the W D bytes of its proof (D of its tree) at
   proofs + k proof_stride; nothing else in a row is touched and the rows
   of a refused tree are not touched.  proof_stride is a multiple of 4 and
   at least W ceil( log2( min( leaf_max, n_leaves ) ) ), the base is 4-byte
   aligned and not NULL where there are leaves; otherwise
   FD_ED25519_ERR_ARG.  Roots, codes and return values are the roots
   calls'; the host version also returns FD_ED25519_ERR_ARG where its
   per-thread layer buffers cannot be allocated. */
int
fd_bmtree_proofs_batch( unsigned                     width,
                        unsigned                     flags,
                        unsigned long                n_trees,
                        uint32_t const *             leaf_cnt,
                        fd_bmtree_gpu_leaf_t const * leaves,
                        void const *                 blob,
                        unsigned long                blob_sz,
                        unsigned long                leaf_max,
                        void *                       roots_out,
                        int *                        codes_out,
                        void *                       proofs_out,
                        unsigned long                proof_stride,
                        int                          nthreads );

int
fd_bmtree_gpu_proofs_packed( fd_ed25519_gpu_t *           gpu,
                             unsigned                     width,
                             unsigned                     flags,
                             unsigned long                n_trees,
                             uint32_t const *             leaf_cnt,
                             fd_bmtree_gpu_leaf_t const * leaves,
                             void const *                 blob,
                             unsigned long                blob_sz,
                             unsigned long                leaf_max,
                             void *                       roots_out,
                             int *                        codes_out,
                             void *                       proofs_out,
                             unsigned long                proof_stride );

/* d_proofs = d_shreds + merkle_off with proof_stride the shred size drops
   each proof into its shred's tail.  d_work is fd_bmtree_gpu_work_sz(
   n_trees, n_leaves ) bytes as for the roots call: the layers are gathered
   from between the merge launches (one gather launch before each), and
   nothing is read back. */
int
fd_bmtree_gpu_proofs_dev( fd_ed25519_gpu_t *           gpu,
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
                          void *                       d_proofs,
                          unsigned long                proof_stride,
                          int *                        d_codes,
                          void *                       d_work,
                          void *                       stream );

/* Verify: the root a leaf and its proof lead to.  Every offset is into the
   call's blob. */
typedef struct {
  uint32_t leaf_off, leaf_sz;   /* the leaf's data, or with FD_BMTREE_GPU_LEAVES_ARE_NODES a ready node (leaf_sz == width) */
  uint32_t proof_off;           /* depth nodes of width bytes, packed, any alignment */
  uint32_t idx;                 /* the leaf's index in its tree */
  uint32_t leaf_cnt;            /* 0: not known (plain walk); else strict walk */
  uint32_t depth;
  uint32_t expect_off;          /* read only with FD_BMTREE_GPU_PROOF_EXPECT */
  uint32_t flags;               /* FD_BMTREE_GPU_PROOF_EXPECT; other bits refuse */
} fd_bmtree_gpu_proof_t;

/* compare the derived root with blob[expect_off, expect_off+W) */
#define FD_BMTREE_GPU_PROOF_EXPECT (1U)

/* Proof i's derived root goes to roots_out + 32 i (a W = 20 root is
   followed by 12 zero bytes); codes_out[i] is 0, FD_BMTREE_ERR_PROOF (only
   with FD_BMTREE_GPU_PROOF_EXPECT: the derived root, which is still
   written, differs from the expected one) or FD_ED25519_ERR_ARG for a
   refused descriptor, which is never hashed, of which nothing is
   dereferenced and whose root is 32 zero bytes:
     a leaf, proof (depth W bytes) or expect range past blob_sz or wrapping
       32 bits,
     leaf_sz > FD_BMTREE_GPU_LEAF_SZ_MAX, in node mode leaf_sz != width,
     depth > depth_max (1..32; it bounds a lane's work as leaf_max does),
     unknown flag bits,
     leaf_cnt == 0: depth < 32 and idx >> depth != 0,
     leaf_cnt != 0: idx >= leaf_cnt or depth != ceil( log2( leaf_cnt ) ).
   A refused descriptor does not disturb its neighbours.  Returns 0 or
   FD_ED25519_ERR_ARG (NULL array, width, unknown call flags, depth_max, n
   past FD_BMTREE_GPU_LEAVES_MAX, thread count). */
int
fd_bmtree_from_proofs_batch( unsigned                      width,
                             unsigned                      flags,
                             unsigned long                 n,
                             fd_bmtree_gpu_proof_t const * proofs,
                             void const *                  blob,
                             unsigned long                 blob_sz,
                             unsigned long                 depth_max,
                             void *                        roots_out,
                             int *                         codes_out,
                             int                           nthreads );

/* The same on the device, synchronous, host buffers: call-level errors as
   for fd_bmtree_gpu_roots_packed (blob_sz >= 2^32 is FD_ED25519_ERR_ARG; on
   FD_ED25519_ERR_GPU nothing is written; no host fallback). */
int
fd_bmtree_gpu_from_proofs_packed( fd_ed25519_gpu_t *            gpu,
                                  unsigned                      width,
                                  unsigned                      flags,
                                  unsigned long                 n,
                                  fd_bmtree_gpu_proof_t const * proofs,
                                  void const *                  blob,
                                  unsigned long                 blob_sz,
                                  unsigned long                 depth_max,
                                  void *                        roots_out,
                                  int *                         codes_out );

/* Device-resident: one launch on `stream` (NULL: the engine's tree stream),
   no work memory, no host synchronisation.  Root i goes to d_roots + i
   root_stride under fd_bmtree_gpu_roots_dev's alignment rules; d_proofs is
   4-byte aligned.  d_roots may point into a part of d_blob that no
   descriptor reads: the roots are then messages in place for
   fd_ed25519_gpu_verify_dev on the same stream (a stream of the caller's:
   with NULL each of the two calls takes a stream of its own unit and they
   are not ordered). */
int
fd_bmtree_gpu_from_proofs_dev( fd_ed25519_gpu_t *            gpu,
                               unsigned                      width,
                               unsigned                      flags,
                               unsigned long                 n,
                               fd_bmtree_gpu_proof_t const * d_proofs,
                               void const *                  d_blob,
                               unsigned long                 blob_sz,
                               unsigned long                 depth_max,
                               void *                        d_roots,
                               unsigned long                 root_stride,
                               int *                         d_codes,
                               void *                        stream );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_bmtree_gpu_h */
