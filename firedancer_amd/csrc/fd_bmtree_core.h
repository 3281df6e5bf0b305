#ifndef HEADER_fd_bmtree_core_h
#define HEADER_fd_bmtree_core_h

/* fd_bmtree_core.h -- the SHA-256 bodies of the binary Merkle tree
   (reference src/ballet/bmtree/fd_bmtree_tmpl.c), built on fd_poh_core.h's
   compression and shared by the host routines (fd_bmtree_host.c) and the
   device kernels (fd_bmtree_gpu_kernels.hip).

     leaf  : SHA-256( 0x00 || data )            any data_sz
     branch: SHA-256( 0x01 || a[0,W) || b[0,W) ) truncated to W in {20, 32}

   A node is eight host-order words (word j = bytes 4j..4j+3, big-endian);
   a 20-byte node uses words 0..4.  Every message starts with one prefix
   byte, so the words of the data sit one byte off word alignment: word k
   of a block is the last byte of data word k-1 and the first three of data
   word k, one funnel shift (v_alignbit_b32 on the device).  The fixed
   shapes are specialised the way fd_poh_step / fd_poh_mix are:

     fd_bmtree_merge20: 41 bytes, one block, the padding literal
     fd_bmtree_hash65 : 65 bytes (the merge of W = 32 and the leaf of a
                        64-byte signature): two blocks, the second one data
                        byte and literal padding, which fold into its
                        unrolled schedule

   fd_bmtree_leaf is the general leaf: any size, any start alignment, bytes
   loaded one by one as in fd_poh_load.

   static inline, C and C++, no libc, no memory besides the arguments. */

#include "fd_poh_core.h"

#define FD_BMTREE_FN FD_POH_CORE_FN

/* ( hi << 24 ) | ( lo >> 8 ): the word that starts one byte before lo */
#if defined(__HIP_DEVICE_COMPILE__)
#define FD_BMTREE_FUN8(hi,lo) __builtin_amdgcn_alignbit( (hi), (lo), 8U )
#else
#define FD_BMTREE_FUN8(hi,lo) ( ((uint32_t)(hi) << 24) | ((uint32_t)(lo) >> 8) )
#endif

FD_BMTREE_FN void fd_bmtree_iv( uint32_t s[8] ) {
  s[0] = FD_POH_IV0; s[1] = FD_POH_IV1; s[2] = FD_POH_IV2; s[3] = FD_POH_IV3;
  s[4] = FD_POH_IV4; s[5] = FD_POH_IV5; s[6] = FD_POH_IV6; s[7] = FD_POH_IV7;
}

/* words big-endian words from 4*words bytes at any alignment */
FD_BMTREE_FN void fd_bmtree_load( uint32_t * d, uint8_t const * p, int words ) {
  for( int j=0; j<words; j++ )
    d[j] = ((uint32_t)p[4*j] << 24) | ((uint32_t)p[4*j+1] << 16) | ((uint32_t)p[4*j+2] << 8) | (uint32_t)p[4*j+3];
}

/* s <- SHA-256( prefix || d[0..15] as 64 big-endian bytes ), prefix a byte value */
FD_BMTREE_FN void fd_bmtree_hash65( uint32_t s[8], uint32_t prefix, uint32_t const d[16] ) {
  uint32_t w[16];
  w[0] = FD_BMTREE_FUN8( prefix, d[0] );
  for( int k=1; k<16; k++ ) w[k] = FD_BMTREE_FUN8( d[k-1], d[k] );
  fd_bmtree_iv( s );
  fd_poh_compress( s, w );
  w[0] = ( d[15] << 24 ) | 0x00800000U;
  w[1] = 0U; w[2] = 0U; w[3] = 0U; w[4] = 0U; w[5] = 0U; w[6] = 0U; w[7] = 0U;
  w[8] = 0U; w[9] = 0U; w[10] = 0U; w[11] = 0U; w[12] = 0U; w[13] = 0U; w[14] = 0U; w[15] = 520U;
  fd_poh_compress( s, w );
}

/* the leaf node of a 64-byte signature, d its sixteen big-endian words */
FD_BMTREE_FN void fd_bmtree_leaf64( uint32_t s[8], uint32_t const d[16] ) { fd_bmtree_hash65( s, 0U, d ); }

/* s <- the 32-byte branch node of a and b (s may not alias a or b) */
FD_BMTREE_FN void fd_bmtree_merge32( uint32_t s[8], uint32_t const a[8], uint32_t const b[8] ) {
  uint32_t d[16];
  for( int k=0; k<8; k++ ) { d[k] = a[k]; d[8+k] = b[k]; }
  fd_bmtree_hash65( s, 1U, d );
}

/* s <- SHA-256( 0x01 || a[0,20) || b[0,20) ): the 20-byte branch node is
   s[0..4] (s may not alias a or b) */
FD_BMTREE_FN void fd_bmtree_merge20( uint32_t s[8], uint32_t const a[5], uint32_t const b[5] ) {
  uint32_t w[16];
  w[0] = FD_BMTREE_FUN8( 1U, a[0] );
  for( int k=1; k<5; k++ ) w[k]   = FD_BMTREE_FUN8( a[k-1], a[k] );
  w[5] = FD_BMTREE_FUN8( a[4], b[0] );
  for( int k=1; k<5; k++ ) w[5+k] = FD_BMTREE_FUN8( b[k-1], b[k] );
  w[10] = ( b[4] << 24 ) | 0x00800000U;
  w[11] = 0U; w[12] = 0U; w[13] = 0U; w[14] = 0U; w[15] = 328U;
  fd_bmtree_iv( s );
  fd_poh_compress( s, w );
}

/* byte m of the padded message 0x00 || p[0,n-1) (n message bytes), the
   length field excluded */
FD_BMTREE_FN uint32_t fd_bmtree_msg_byte( uint8_t const * p, uint32_t n, uint32_t m ) {
  if( m < n ) return m ? (uint32_t)p[m-1U] : 0U;
  return m == n ? 0x80U : 0U;
}

/* s <- SHA-256( 0x00 || p[0,sz) ), sz < 2^29 - 1.  Whole blocks take four
   byte loads per word; the last one or two blocks (data tail, 0x80,
   zeros, bit length) are formed byte by byte. */
FD_BMTREE_FN void fd_bmtree_leaf( uint32_t s[8], uint8_t const * p, uint32_t sz ) {
  uint32_t n    = sz + 1U;
  uint32_t full = n >> 6;
  uint32_t w[16];
  fd_bmtree_iv( s );
  for( uint32_t blk=0U; blk<full; blk++ ) {
    uint8_t const * q = p + ( blk << 6 );         /* q[-1] (blk > 0) is message byte 64 blk */
    w[0] = ( blk ? (uint32_t)p[(blk<<6)-1U] << 24 : 0U ) | ((uint32_t)q[0] << 16) | ((uint32_t)q[1] << 8) | (uint32_t)q[2];
    for( int k=1; k<16; k++ )
      w[k] = ((uint32_t)q[4*k-1] << 24) | ((uint32_t)q[4*k] << 16) | ((uint32_t)q[4*k+1] << 8) | (uint32_t)q[4*k+2];
    fd_poh_compress( s, w );
  }
  uint32_t m0 = full << 6;
  for( int k=0; k<16; k++ ) {
    uint32_t m = m0 + 4U*(uint32_t)k;
    w[k] = ( fd_bmtree_msg_byte( p, n, m ) << 24 ) | ( fd_bmtree_msg_byte( p, n, m+1U ) << 16 )
         | ( fd_bmtree_msg_byte( p, n, m+2U ) << 8 ) | fd_bmtree_msg_byte( p, n, m+3U );
  }
  if( n - m0 >= 56U ) {                           /* no room for the length: a block of its own */
    fd_poh_compress( s, w );
    for( int k=0; k<16; k++ ) w[k] = 0U;
  }
  w[15] = n << 3;
  fd_poh_compress( s, w );
}

/* Inclusion proofs (include/fd_bmtree_gpu.h).  A tree of c leaves has
   depth ceil( log2( c ) ) and ceil( c / 2^l ) nodes in layer l; the proof
   of leaf i holds, for each layer l below the root, the sibling ( i >> l ) ^ 1
   of the node on its path, or that node itself where the layer ends before
   the sibling (the node that is merged with itself). */

/* ceil( log2( n ) ), 0 for n <= 1 */
FD_BMTREE_FN uint32_t fd_bmtree_depth( uint32_t n ) {
  uint32_t l = 0U;
  while( l < 32U && ( (uint64_t)1 << l ) < (uint64_t)n ) l++;
  return l;
}

/* the nodes of layer l <= 32 of a tree of c leaves */
FD_BMTREE_FN uint32_t fd_bmtree_layer_cnt( uint32_t c, uint32_t l ) {
  return (uint32_t)( ( (uint64_t)c + ( (uint64_t)1 << l ) - 1UL ) >> l );
}

/* node j of a layer of cl nodes has no sibling */
FD_BMTREE_FN int fd_bmtree_no_sibling( uint32_t j, uint32_t cl ) { return ( j ^ 1U ) >= cl; }

/* the node of a layer of cl nodes that the proof of a leaf below node j holds */
FD_BMTREE_FN uint32_t fd_bmtree_proof_idx( uint32_t j, uint32_t cl ) { return fd_bmtree_no_sibling( j, cl ) ? j : ( j ^ 1U ); }

/* One step of the walk at width W: node <- merge( p, node ) where the node
   is a right child, merge( node, p ) where it is a left one, and
   merge( node, node ) where it has no sibling (p is not read). */
FD_BMTREE_FN void fd_bmtree_walk_step( uint32_t W, uint32_t node[8], uint32_t const * p, uint32_t right, int alone ) {
  uint32_t a[8], b[8], s[8];
  int words = W == 32U ? 8 : 5;
  for( int k=0; k<words; k++ ) {
    uint32_t sib = alone ? node[k] : p[k];
    a[k] = right ? sib : node[k];
    b[k] = right ? node[k] : sib;
  }
  if( W == 32U ) fd_bmtree_merge32( s, a, b ); else fd_bmtree_merge20( s, a, b );
  for( int k=0; k<words; k++ ) node[k] = s[k];
}

/* One proof descriptor against the header's refusal rules: nonzero where it
   may be walked.  nodes: the leaf is a ready node; sz_max the leaf size
   limit; expect: the descriptor's flags ask for the comparison. */
FD_BMTREE_FN int fd_bmtree_proof_ok( uint32_t W, int nodes, uint64_t blob_sz, uint32_t depth_max, uint32_t sz_max,
                                     uint32_t leaf_off, uint32_t leaf_sz, uint32_t proof_off, uint32_t idx, uint32_t leaf_cnt,
                                     uint32_t depth, uint32_t expect_off, uint32_t flags ) {
  uint64_t lim = blob_sz < 0xffffffffUL ? blob_sz : 0xffffffffUL;
  if( flags & ~1U ) return 0;
  if( depth > depth_max || depth > 32U ) return 0;
  if( (uint64_t)leaf_off + (uint64_t)leaf_sz > lim ) return 0;
  if( leaf_sz > sz_max || ( nodes && leaf_sz != W ) ) return 0;
  if( (uint64_t)proof_off + (uint64_t)depth * (uint64_t)W > lim ) return 0;
  if( ( flags & 1U ) && (uint64_t)expect_off + (uint64_t)W > lim ) return 0;
  if( !leaf_cnt ) return depth >= 32U || !( idx >> depth );
  return idx < leaf_cnt && depth == fd_bmtree_depth( leaf_cnt );
}

#endif /* HEADER_fd_bmtree_core_h */
