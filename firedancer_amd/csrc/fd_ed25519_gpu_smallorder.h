/* fd_ed25519_gpu_smallorder.h -- the reference's small-order test
   (fd_ed25519_ge_p3_is_small_order, src/ballet/ed25519/fd_ed25519_ge.c:
   21-66) as a classifier on the 32 encoding bytes.

   The reference triples-doubles the decompressed point and compares the
   limbs of [8]P with the identity's (is_identity, fd_ed25519_ge.c:41-59).
   Its verdict is a pure function of the encoding, and that function has
   exactly 14 ones:

     - limb equality implies value equality, so a flagged point has
       [8]P = O: it is one of the curve's 8 torsion points, whose y are
       0, 1, -1, y8 and -y8 (mod p);
     - the lax decoder (fd_ed25519_fe_frombytes) ignores bit 255
       as a value bit and accepts y >= p, so a 255-bit y field decodes to
       one of those five values only if it is 0, 1, p-1, y8, p-y8, p or
       p+1 (every other representative is >= 2^255); each of the seven
       decodes with either sign bit (x = 0 is its own negative), which
       gives corpus.small_order_encodings(), 14 encodings;
     - the reference flags every one of those 14 (they decode to fixed
       limbs, so this is a finite check: tests/test_small_order_table.py
       runs it against the reference build together with their 3,584
       single-bit flips, y + p for small y and random encodings).

   So the flag is FD_PT_SMALL iff the y field is one of the seven words
   below, whatever the sign bit: 8 word compares per constant instead of 3
   doublings, 9 conversion multiplies and 4 identity multiplies per point.
   Callers apply it only to encodings that decoded (an off-curve y field
   is none of the seven anyway). */

#ifndef FD_ED25519_GPU_SMALLORDER_H
#define FD_ED25519_GPU_SMALLORDER_H

#include "fd_ed25519_gpu_fe.h"

#define FD_SMALL_ORDER_Y_CNT 7

/* y fields (bit 255 cleared) as 8 little-endian words: 0, 1, p-y8, y8,
   p-1, p, p+1 */
static constexpr uint32_t fd_small_order_y[FD_SMALL_ORDER_Y_CNT][8] = {
  { 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u },
  { 0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u },
  { 0x8f95e826u, 0xb027b2c2u, 0x89f4c345u, 0xf098eff2u, 0x05acdfd5u, 0x3933c6d3u, 0x880238b1u, 0x05fc536du },
  { 0x706a17c7u, 0x4fd84d3du, 0x760b3cbau, 0x0f67100du, 0xfa53202au, 0xc6cc392cu, 0x77fdc74eu, 0x7a03ac92u },
  { 0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu },
  { 0xffffffedu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu },
  { 0xffffffeeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu } };

/* 1 iff the encoding w (8 little-endian words) is one of the 14
   small-order encodings */
FD_DEV int fd_enc_is_small_order( uint32_t const (&w)[8] ) {
  uint32_t const w7 = w[7] & 0x7fffffffu;
  int hit = 0;
#pragma unroll
  for( int c=0; c<FD_SMALL_ORDER_Y_CNT; c++ ) {
    uint32_t d = w7 ^ fd_small_order_y[c][7];
#pragma unroll
    for( int k=0; k<7; k++ ) d |= w[k] ^ fd_small_order_y[c][k];
    hit |= (d == 0u);
  }
  return hit;
}

#endif /* FD_ED25519_GPU_SMALLORDER_H */
