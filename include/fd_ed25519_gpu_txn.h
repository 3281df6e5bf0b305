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
   entries and results; and, for every ring slot, the scratch of the ring's
   transaction batches (fd_ed25519_gpu_submit_txns below: max_sigs
   descriptors and results in HBM and max_sigs pinned results, whatever
   max_txn is).  A tile calls it before sandboxing; without it the
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

/* Transactions through the pinned ring: the asynchronous form, on the same
   slots, tickets, staging, registered-region DMA and CU groups as
   fd_ed25519_gpu_submit / _try_submit / _poll (fd_ed25519_gpu.h).  Only
   the ring lock is taken; several batches are in flight at once, each on
   its slot's own scratch.

   Claimed slots.  A ring batch's slot layout is computed by the host, from
   the one byte a payload that parses cannot contradict, its first
   (fd_txn_parse takes signature_cnt from it and rejects anything outside
   [1, 127]):

     claim(t) = blob[ txn[t].off ]  if the entry lies inside blob[0, blob_sz),
                                    has sz >= 1 and that byte is in [1, 127],
              = 0                   otherwise;
     base(t)  = the sum of claim(u) over u < t;   n_sig = the sum over all t.

   Transaction t owns slots [base(t), base(t) + claim(t)) and the verify
   pipeline runs on exactly n_sig slots: no scan on the device, no tail.  A
   transaction that parses has sig_cnt == claim(t).  One that claims slots
   but does not parse keeps them: they hold the fill descriptor (sig_off =
   pub_off = 0xffffffff; their codes are FD_ED25519_ERR_ARG), its status is
   FD_ED25519_ERR_TXN with the parser's reject_line, and sig_cnt, tag and
   footprint are 0 as everywhere else.

   This is the one difference from fd_ed25519_gpu_verify_txns_dev and
   _packed: on the ring, sig_base is base(t) as defined here, so an
   unparsed transaction with a nonzero claim does take slots, and the
   per-signature codes are indexed by the claim prefix, not by the prefix
   of the parsed counts.  Every other field is the same. */

/* bases[0..n_txn] <- the exclusive prefix of the claims, bases[n_txn] =
   n_sig; returns n_sig (as an unsigned long: the prefix itself is 32 bits,
   enough for the 2^24 transactions of 127 signatures a launch is bounded
   by).  bases may be NULL: the total only.  Pure host code, no engine, no
   device: a tile closes a batch with it when the total would pass the
   engine's max_sigs. */
unsigned long
fd_ed25519_gpu_txn_claims( void const *                 blob,
                           unsigned long                blob_sz,
                           fd_ed25519_gpu_txn_t const * txn,
                           unsigned long                n_txn,
                           uint32_t *                   bases );

/* Submit one batch: 1 submitted (*ticket set), 0 the ring is full (poll
   first), < 0 an error.  FD_ED25519_ERR_ARG, with nothing queued and every
   slot as it was: n_txn == 0 or > max_sigs, n_sig (the claimed total) >
   max_sigs, blob_sz > max_blob, a NULL ticket, txn or (blob_sz != 0) blob.
   A batch in which nothing claims a slot is valid: the parser runs alone.

   blob is used as fd_ed25519_gpu_try_submit uses it: read in place by DMA
   if it lies in a region given to fd_ed25519_gpu_register, taken as it
   lies if it is a slot's staged buffer (fd_ed25519_gpu_stage; the stage is
   released on every return that reached a slot, as fd_ed25519_gpu_
   try_submit2 releases it), copied into a slot's pinned buffer otherwise;
   txn is copied during the call.  The engine's mode and schedule knobs
   apply as to any ring batch, and the CU-group rule with n = n_sig.
   Without fd_ed25519_gpu_txns_reserve the first submit allocates the
   slots' scratch. */
int
fd_ed25519_gpu_try_submit_txns( fd_ed25519_gpu_t *           gpu,
                                unsigned long                n_txn,
                                void const *                 blob,
                                unsigned long                blob_sz,
                                fd_ed25519_gpu_txn_t const * txn,
                                unsigned long *              ticket );

/* The same; 0, or FD_ED25519_ERR_ARG when the ring is full, as
   fd_ed25519_gpu_submit. */
int
fd_ed25519_gpu_submit_txns( fd_ed25519_gpu_t *           gpu,
                            unsigned long                n_txn,
                            void const *                 blob,
                            unsigned long                blob_sz,
                            fd_ed25519_gpu_txn_t const * txn,
                            unsigned long *              ticket );

/* Collect a transaction ticket: res takes the batch's n_txn results,
   codes_opt (NULL, or n_sig ints) the per-signature codes by claimed slot.
   block as fd_ed25519_gpu_poll's: bit 0 waits (bounded by the engine's
   timeout), FD_ED25519_GPU_POLL_KEEP leaves the slot's pinned buffers
   staged to the caller.  Returns 1 collected, 0 not ready, < 0 an error
   (the ticket stays valid).  Tickets come from the engine's one counter:
   this call on a descriptor ticket, and fd_ed25519_gpu_poll with out !=
   NULL on a transaction ticket, return FD_ED25519_ERR_ARG and leave the
   ticket as it was; fd_ed25519_gpu_poll( gpu, ticket, NULL, block ) drains
   either kind. */
int
fd_ed25519_gpu_poll_txns( fd_ed25519_gpu_t *            gpu,
                          unsigned long                 ticket,
                          fd_ed25519_gpu_txn_result_t * res,
                          int *                         codes_opt,
                          int                           block );

/* Diagnostics: the number of ring slots whose transaction scratch has been
   allocated so far (0, then the ring's depth after fd_ed25519_gpu_
   txns_reserve or the first submit; it never moves afterwards). */
unsigned long
fd_ed25519_gpu_txn_ring_allocs( fd_ed25519_gpu_t * gpu );

/* Diagnostics (tools/txn_bench.py --ring): one batch submitted and polled,
   with HIP events around fd_k_txn_ring_front and fd_k_txn_ring_reduce;
   their durations (ms) go to kernel_ms[2].  One caller at a time. */
int
fd_ed25519_gpu_txn_ring_timed( fd_ed25519_gpu_t *            gpu,
                               unsigned long                 n_txn,
                               void const *                  blob,
                               unsigned long                 blob_sz,
                               fd_ed25519_gpu_txn_t const *  txn,
                               fd_ed25519_gpu_txn_result_t * res,
                               float *                       kernel_ms );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_gpu_txn_h */
