/* fd_sha512_gpu_pack.h -- the host side of the long SHA-512 / SHA-384 path
   (fd_sha512_gpu_long, fd_ed25519_gpu_host.cpp): the padded byte stream of a
   message and the geometry of the pinned blob it is moved through.  Plain
   C / C++ with no HIP in it, so a stand-alone host program can include it
   (tests/sha_long_pack_harness.cpp runs it under the sanitizers). */
#ifndef FD_SHA512_GPU_PACK_H
#define FD_SHA512_GPU_PACK_H

#include <stdint.h>
#include <string.h>

/* one lane's work of one launch (fd_k_sha512_pieces): nblk consecutive
   128-byte blocks of its message's padded stream, staged at data + off */
typedef struct { uint64_t off; uint32_t nblk; uint32_t flags; } fd_sha_lpiece_t;
#define FD_SHA_PIECE_FIRST 1U   /* start from the IV, not from the lane's state row */
#define FD_SHA_PIECE_LAST  2U   /* the stream ends here: the row receives the big-endian digest */
#define FD_SHA_PIECE_384   4U   /* the SHA-384 IV, and 6 digest words */

/* messages hashed side by side are capped as in the verify long path */
#define FD_SHA_LONG_GROUP_MAX 4096UL

/* 128-byte blocks of the padded stream M || 0x80 || 0.. || bitlen128 of a
   message of sz bytes (no sz overflows it) */
static inline unsigned long fd_sha_long_blocks( unsigned long sz ) {
  return ( sz >> 7 ) + 1UL + ( ( sz & 127UL ) >= 112UL ? 1UL : 0UL );
}

/* bytes [pos, pos+len) of that stream into dst; pos + len at most 128
   fd_sha_long_blocks( sz ).  msg + x is formed and read for x < sz only:
   a range at or past the message's end never touches msg (which may then
   be NULL).  The bit count is 128 bits wide, its high word sz >> 61. */
static inline void fd_sha_long_pack( uint8_t * dst, uint8_t const * msg, unsigned long sz, unsigned long pos, unsigned long len ) {
  unsigned long x = pos, left = len;
  if( x < sz && left ) {
    unsigned long k = sz - x < left ? sz - x : left;
    memcpy( dst, msg + x, k );
    dst += k; x += k; left -= k;
  }
  if( !left ) return;
  memset( dst, 0, left );
  if( x == sz ) dst[0] = 0x80;                               /* the padding bit */
  unsigned long nb = fd_sha_long_blocks( sz );
  if( ( x + left ) >> 7 == nb && !( ( x + left ) & 127UL ) ) {   /* the stream's end: the bit count's bytes that fall in range */
    unsigned long hi = sz >> 61, lo = sz << 3;
    unsigned long cnt = left < 16UL ? left : 16UL;           /* a range may begin inside the count */
    for( unsigned long b=16UL-cnt; b<16UL; b++ ) {           /* byte b of the count sits 16 - b before the end */
      unsigned long v = b < 8UL ? hi >> ( 8UL*( 7UL - b ) ) : lo >> ( 8UL*( 15UL - b ) );
      dst[ left - ( 16UL - b ) ] = (uint8_t)v;
    }
  }
}

/* How a group of m messages goes through a pinned blob of max_blob bytes:
   nhalf buffers (2: ping-pong; 1: the blob is too small for two), buffer h
   at byte half_off[h], each m C 128 data bytes (message j's C blocks at
   j C 128) followed by m piece entries. */
typedef struct {
  unsigned long G;            /* messages per group at most */
  unsigned long C;            /* blocks per message per launch, >= 1 */
  unsigned long nhalf;        /* 1 or 2 */
  unsigned long half_sz;      /* m ( 128 C + 16 ) */
  unsigned long half_off[2];
} fd_sha_long_geom_t;

/* Returns 0 and fills geo, or -1: the blob cannot hold one 128-byte block
   and its 16-byte piece entry (max_blob < 144) or max_sigs is 0 -- the only
   failure -- or m is not in [1, G] (G is still written).  pingpong 0 keeps
   one buffer whatever the blob's size. */
static inline int fd_sha_long_geom( unsigned long max_blob, unsigned long max_sigs, unsigned long m, int pingpong,
                                    fd_sha_long_geom_t * geo ) {
  unsigned long const ent = 128UL + sizeof(fd_sha_lpiece_t);
  memset( geo, 0, sizeof(*geo) );
  unsigned long nhalf = pingpong && max_blob / ( 2UL*ent ) ? 2UL : 1UL;
  unsigned long G = max_blob / ( nhalf*ent );
  if( G > max_sigs ) G = max_sigs;
  if( G > FD_SHA_LONG_GROUP_MAX ) G = FD_SHA_LONG_GROUP_MAX;
  geo->G = G;
  if( !G || !m || m > G ) return -1;
  geo->nhalf       = nhalf;
  geo->C           = ( max_blob / ( nhalf*m ) - sizeof(fd_sha_lpiece_t) ) / 128UL;
  geo->half_sz     = m * ( 128UL*geo->C + sizeof(fd_sha_lpiece_t) );
  geo->half_off[0] = 0UL;
  geo->half_off[1] = nhalf > 1UL ? geo->half_sz : 0UL;
  return 0;
}

#endif
