#ifndef HEADER_fd_ed25519_gpu_txn_h
#define HEADER_fd_ed25519_gpu_txn_h

/* fd_ed25519_gpu_txn.h -- whole transactions on the GPU engine: payloads
   in, one verdict and a dedup tag per transaction out.

   The engine's other entry points take one fd_ed25519_gpu_desc_t per
   signature, which a host builds by parsing each payload (fd_txn_parse)
   and expanding it into signature_cnt descriptors, and give back one code
   per signature, which the host folds into "publish or filter".  Here all
   of that runs on the device:

     fd_k_txn_parse   one lane per transaction runs the parser core
                      (fd_txn_core.h: fd_txn_parse's acceptance rules),
     fd_k_txn_scan    an exclusive scan of the signature counts gives each
                      transaction its first slot, sig_base,
     fd_k_txn_expand  slot sig_base + i becomes the descriptor of signature
                      i over the message with signer account i,
     the verify pipeline (fd_ed25519_gpu_verify_dev, unchanged) on those
                      descriptors,
     fd_k_txn_reduce  the first nonzero code of a transaction's slots in
                      signature order becomes its status (the
                      fd_ed25519_verify_batch_single_msg rule).

   The host never learns the signature total before it launches the verify
   pipeline: it launches it on a bound (sig_cap; the packed call's is the
   total the payloads' first bytes claim) and fd_k_txn_expand fills the
   slots past the real total with a descriptor that fails the device's own
   bounds check (sig_off = pub_off = 0xffffffff), which fd_k_prep reports
   as FD_ED25519_ERR_ARG without dereferencing it (fd_ed25519_gpu.h,
   "Descriptor bounds").  fd_k_txn_reduce never looks at those slots. */

#include "fd_ed25519_gpu.h"
#include "fd_txn_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The payload could not be parsed: fd_txn_parse would return 0.  An engine
   code, as FD_ED25519_ERR_ARG and FD_ED25519_ERR_GPU are. */
#define FD_ED25519_ERR_TXN (-18)

typedef struct { uint32_t off, sz; } fd_ed25519_gpu_txn_t;      /* payload = blob[off, off+sz) */

typedef struct {                                                /* 24 bytes */
  int32_t  status;      /* see below */
  uint32_t sig_base;    /* index of its signature 0 in the per-signature arrays */
  uint64_t tag;         /* first 8 bytes of signature 0 (the tile's dedup tag); 0 if malformed */
  uint16_t footprint;   /* fd_txn_parse's return value; 0 if malformed */
  uint16_t reject_line; /* the reference line fd_txn_parse records for the rejection; 0 if parsed */
  uint8_t  sig_cnt;     /* 0 if malformed */
  uint8_t  version;     /* FD_TXN_VLEGACY / FD_TXN_V0 */
  uint8_t  _pad[2];     /* zero */
} fd_ed25519_gpu_txn_result_t;

/* status:
     FD_ED25519_SUCCESS     every signature verifies;
     FD_ED25519_ERR_SIG / _PUBKEY / _MSG
                            the first nonzero per-signature code in
                            signature order: the code of signature i over
                            payload[message_off, sz) with signer account i,
                            under the engine's current mode;
     FD_ED25519_ERR_TXN     fd_txn_parse would return 0 (reject_line says
                            why);
     FD_ED25519_ERR_ARG     the entry's [off, off+sz) does not lie inside
                            blob[0, blob_sz): it is never dereferenced,
                            reject_line is 0 -- or, on the device-resident
                            path, the transaction parsed but its signatures
                            end past sig_cap (below).
   Whatever is not parsed (ERR_TXN, the first kind of ERR_ARG) has tag,
   footprint and sig_cnt 0 and version FD_TXN_VLEGACY, takes no slot, and
   shares the sig_base of the next transaction that takes one.  footprint
   saturates at 65535 (only payloads far past the MTU, tens of kilobytes of
   instructions, reach that; their descriptor is written by its true
   size). */

/* Allocate the engine scratch the calls below need for batches of up to
   max_txn transactions: two sets (successive calls alternate) of
   per-signature descriptors and codes (max_sigs each), per-transaction
   counts and the scan's partial sums, and the packed call's device-side
   entries and results.  A tile calls it before sandboxing; without it the
   first call (and every call with more transactions than any before)
   allocates.  fd_ed25519_gpu_delete frees the scratch.  Returns 0,
   FD_ED25519_ERR_ARG or FD_ED25519_ERR_GPU. */
int
fd_ed25519_gpu_txns_reserve( fd_ed25519_gpu_t * gpu,
                             unsigned long      max_txn );

/* Device-resident: d_blob (blob_sz <= 2^32 - 1 bytes followed by >= 16
   readable pad bytes, as fd_ed25519_gpu_verify_dev), d_txn (n_txn
   entries), d_res (n_txn results, 8-byte aligned), d_codes_opt (NULL or
   sig_cap ints) and d_txn_out_opt (NULL or n_txn * txn_out_stride bytes,
   2-byte aligned; txn_out_stride even and >= 20) are device pointers.

   The stream contract of fd_ed25519_gpu_verify_dev: the work is ordered
   after everything queued on `stream` (NULL: the engine's own) and its
   results are visible to work queued on `stream` afterwards; no host
   synchronisation.  Two calls in a row need no synchronisation between
   them either.

   sig_cap <= max_sigs bounds the batch's signatures.  Transactions are
   given slots in order; one whose last slot would lie at or past sig_cap
   gets FD_ED25519_ERR_ARG (with its parse fields and the sig_base it would
   have had), and so does every parsed transaction after it; those before
   it are unaffected.  sig_cap == 0 runs the parser alone.

   d_codes_opt[sig_base + i] receives the code of signature i of every
   transaction that got slots; entries past the batch's last slot hold
   FD_ED25519_ERR_ARG (the tail slots) or are left alone.

   d_txn_out_opt + t * txn_out_stride receives transaction t's fd_txn_t
   (exactly the bytes fd_txn_parse writes) when it parsed and its footprint
   is at most txn_out_stride; otherwise not a byte is written there, and a
   nonzero footprint tells the caller to parse that one itself.

   Returns 0, FD_ED25519_ERR_ARG (nothing queued) or FD_ED25519_ERR_GPU. */
int
fd_ed25519_gpu_verify_txns_dev( fd_ed25519_gpu_t *            gpu,
                                unsigned long                 n_txn,
                                void const *                  d_blob,
                                unsigned long                 blob_sz,
                                fd_ed25519_gpu_txn_t const *  d_txn,
                                unsigned long                 sig_cap,
                                fd_ed25519_gpu_txn_result_t * d_res,
                                int *                         d_codes_opt,
                                void *                        d_txn_out_opt,
                                unsigned long                 txn_out_stride,
                                void *                        stream );

/* Synchronous, host buffers, blob_sz <= max_blob.  n_txn is not bounded:
   the batch runs as consecutive launches, each of as many transactions as
   claim (by their first payload byte, the signature count) at most
   max_sigs signatures, and no transaction is ever refused for capacity
   (unless max_sigs < 127 and it alone claims more).  sig_base and the
   indices of codes_opt are global across those launches: codes_opt takes
   one int per signature of every parsed transaction (at most the claimed
   total; 127 n_txn always suffices).  res, codes_opt and txn_out_opt as
   d_res, d_codes_opt and d_txn_out_opt above.  Returns 0,
   FD_ED25519_ERR_ARG (nothing sent to the device) or FD_ED25519_ERR_GPU
   (device failure or timeout; nothing written). */
int
fd_ed25519_gpu_verify_txns_packed( fd_ed25519_gpu_t *            gpu,
                                   unsigned long                 n_txn,
                                   void const *                  blob,
                                   unsigned long                 blob_sz,
                                   fd_ed25519_gpu_txn_t const *  txn,
                                   fd_ed25519_gpu_txn_result_t * res,
                                   int *                         codes_opt,
                                   void *                        txn_out_opt,
                                   unsigned long                 txn_out_stride );

/* Diagnostics, in the style of fd_ed25519_gpu_debug_k: parse, scan and
   expand only, with sig_cap slots (<= max_sigs).  desc_out (sig_cap
   entries) receives every slot as fd_k_txn_expand wrote it, tail slots
   included; *n_sig_out the number of slots transactions took; res_opt
   (NULL or n_txn results) the parse fields, status FD_ED25519_SUCCESS
   standing for "parsed, got its slots".  Synchronous, host buffers,
   blob_sz <= max_blob. */
int
fd_ed25519_gpu_debug_txn_descs( fd_ed25519_gpu_t *            gpu,
                                unsigned long                 n_txn,
                                void const *                  blob,
                                unsigned long                 blob_sz,
                                fd_ed25519_gpu_txn_t const *  txn,
                                unsigned long                 sig_cap,
                                fd_ed25519_gpu_desc_t *       desc_out,
                                unsigned long *               n_sig_out,
                                fd_ed25519_gpu_txn_result_t * res_opt );

/* Diagnostics (tools/txn_bench.py): fd_ed25519_gpu_verify_txns_dev with HIP
   events around the four kernels it adds; blocks until the batch is done
   and writes their durations (ms) to kernel_ms[4] in the order parse,
   scan, expand, reduce. */
int
fd_ed25519_gpu_verify_txns_dev_timed( fd_ed25519_gpu_t *            gpu,
                                      unsigned long                 n_txn,
                                      void const *                  d_blob,
                                      unsigned long                 blob_sz,
                                      fd_ed25519_gpu_txn_t const *  d_txn,
                                      unsigned long                 sig_cap,
                                      fd_ed25519_gpu_txn_result_t * d_res,
                                      int *                         d_codes_opt,
                                      void *                        d_txn_out_opt,
                                      unsigned long                 txn_out_stride,
                                      void *                        stream,
                                      float *                       kernel_ms );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_gpu_txn_h */
