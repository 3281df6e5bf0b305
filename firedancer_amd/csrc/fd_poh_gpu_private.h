#ifndef HEADER_fd_poh_gpu_private_h
#define HEADER_fd_poh_gpu_private_h

/* fd_poh_gpu_private.h -- between fd_poh_gpu.cpp (host side) and the
   kernel unit fd_poh_gpu_kernels.hip. */

#include <hip/hip_runtime.h>
#include "fd_poh_gpu.h"

/* A lane's work row, FD_POH_ROW_WORDS words (48 bytes, 16-aligned):
   words 0..7 the state in host order, 8..9 the hashes still to run (low,
   high), 10 FD_POH_ROW_DONE once the entry's code is written, 11 unused.
   Words 8..11 are one 16-byte load: all a done row costs its lane. */
#define FD_POH_ROW_WORDS 12U
#define FD_POH_ROW_DONE  1U

/* One launch of fd_k_poh over lanes [0, lanes): lane i owns entry
   order[i] (order NULL: entry i) and row i of work.  first != 0: the rows
   are written from the entries (and entries the header refuses get their
   FD_ED25519_ERR_ARG here); otherwise a lane continues from its row.  Each
   lane runs min( remaining, chunk ) hashes. */
extern "C" hipError_t fd_poh_gpu_launch( uint32_t lanes, uint32_t first, uint32_t chunk, uint64_t n_max,
                                         fd_poh_gpu_entry_t const * ent, uint32_t const * order, uint32_t * work,
                                         int32_t * out, uint8_t * state_out, hipStream_t stream );

#endif /* HEADER_fd_poh_gpu_private_h */
