// small_order_harness.cpp -- the encoding classifier of
// firedancer_amd/csrc/fd_ed25519_gpu_smallorder.h (__host__ __device__)
// compiled for the host, so tests/test_small_order_table.py can hold it
// against the reference's decompression + small-order test.  Test
// infrastructure only.
#include "fd_ed25519_gpu_smallorder.h"

extern "C" {
/* flag[i] = classifier's verdict on the 32-byte encoding i */
void h_enc_is_small_order( int32_t * flag, uint8_t const * enc, unsigned long n ) {
  for( unsigned long i=0; i<n; i++ ) {
    uint32_t w[8];
    for( int j=0; j<8; j++ )
      w[j] = (uint32_t)enc[32*i+4*j] | ((uint32_t)enc[32*i+4*j+1]<<8) | ((uint32_t)enc[32*i+4*j+2]<<16) | ((uint32_t)enc[32*i+4*j+3]<<24);
    flag[i] = fd_enc_is_small_order( w );
  }
}
/* the constant table, [FD_SMALL_ORDER_Y_CNT][8] little-endian words */
int h_small_order_table( uint32_t * out ) {
  for( int c=0; c<FD_SMALL_ORDER_Y_CNT; c++ ) for( int k=0; k<8; k++ ) out[8*c+k] = fd_small_order_y[c][k];
  return FD_SMALL_ORDER_Y_CNT;
}
}
