/* sha_long_pack_harness.cpp -- the host side of the long SHA-512 path
   (firedancer_amd/csrc/fd_sha512_gpu_pack.h) as a stand-alone program, for
   tests/test_sha512_long_host.py, which builds it with
   -fsanitize=address,undefined and runs it as a child process.

     stream  LO HI CUT [MAX_BLOB MAX_SIGS M]
        for every SZ in [LO, HI] writes to stdout the length (8 bytes,
        little endian) and the bytes of the padded stream of the SZ-byte
        message i -> (i*131+7)&255, packed in pieces.  CUT "128": one piece
        per block; CUT "geo": pieces of C blocks, C from the geometry of
        MAX_BLOB, MAX_SIGS and a group of M (M 0: M = G).  The message is a
        heap block of exactly SZ bytes, so a read one byte past it is caught.
     tail    SZ
        writes the final 128 bytes of the padded stream of an SZ-byte
        message, packed with msg = NULL (SZ a multiple of 128: they hold no
        message byte, and nothing may be dereferenced).
     geometry LO HI
        checks every max_blob in [LO, HI], max_sigs in {1, 8, 64, 4096} and
        m in [1, G], with ping-pong and with one buffer; prints the number
        of (max_blob, max_sigs, m) cases and "geometry ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fd_sha512_gpu_pack.h"

#define CHECK(c) do { if( !(c) ) { fprintf( stderr, "FAIL %s:%d %s (max_blob %lu max_sigs %lu m %lu pp %d)\n", __FILE__, __LINE__, #c, \
                                            max_blob, max_sigs, m, pp ); return 1; } } while(0)

static int geometry( unsigned long lo, unsigned long hi ) {
  static unsigned long const sigs[4] = { 1UL, 8UL, 64UL, 4096UL };
  unsigned long cases = 0UL;
  for( unsigned long max_blob=lo; max_blob<=hi; max_blob++ ) for( int s=0; s<4; s++ ) for( int pp=0; pp<2; pp++ ) {
    unsigned long max_sigs = sigs[s], m = 1UL;
    fd_sha_long_geom_t g;
    int r = fd_sha_long_geom( max_blob, max_sigs, 1UL, pp, &g );
    unsigned long G = g.G;
    CHECK( ( max_blob >= 144UL ) == ( r == 0 ) );            /* the only failure: no room for a block and its entry */
    if( r ) { CHECK( G == 0UL ); continue; }
    CHECK( G >= 1UL && G <= max_sigs && G <= 4096UL );
    for( m=1UL; m<=G; m++ ) {
      CHECK( !fd_sha_long_geom( max_blob, max_sigs, m, pp, &g ) );
      CHECK( g.G == G && g.C >= 1UL );
      CHECK( g.nhalf == ( pp && max_blob >= 288UL ? 2UL : 1UL ) );
      CHECK( g.half_sz == m * ( g.C * 128UL + 16UL ) );
      for( unsigned long h=0; h<g.nhalf; h++ ) {
        CHECK( g.half_off[h] == h * g.half_sz );
        CHECK( g.half_off[h] + g.half_sz <= max_blob );      /* data and piece table inside the blob */
        for( unsigned long j=0; j<m; j++ ) CHECK( !( ( g.half_off[h] + j * g.C * 128UL ) & 15UL ) );
        CHECK( !( ( g.half_off[h] + m * g.C * 128UL ) & 15UL ) );
      }
      /* C is the largest that fits */
      CHECK( g.nhalf * m * ( ( g.C + 1UL ) * 128UL + 16UL ) > max_blob );
      if( pp ) cases++;
    }
    m = G + 1UL;
    CHECK( fd_sha_long_geom( max_blob, max_sigs, m, pp, &g ) == -1 && g.G == G );
    m = 0UL;
    CHECK( fd_sha_long_geom( max_blob, max_sigs, m, pp, &g ) == -1 );
  }
  printf( "%lu cases\ngeometry ok\n", cases );
  return 0;
}

int main( int argc, char ** argv ) {
  if( argc == 4 && !strcmp( argv[1], "geometry" ) ) return geometry( strtoul( argv[2], NULL, 0 ), strtoul( argv[3], NULL, 0 ) );
  if( argc == 3 && !strcmp( argv[1], "tail" ) ) {
    unsigned long sz = strtoul( argv[2], NULL, 0 );
    if( sz & 127UL ) return 2;
    uint8_t out[128];
    memset( out, 0xEE, sizeof(out) );
    fd_sha_long_pack( out, NULL, sz, ( fd_sha_long_blocks( sz ) - 1UL ) * 128UL, 128UL );
    return fwrite( out, 1, 128, stdout ) == 128 ? 0 : 1;
  }
  if( ( argc == 5 || argc == 8 ) && !strcmp( argv[1], "stream" ) ) {
    unsigned long lo = strtoul( argv[2], NULL, 0 ), hi = strtoul( argv[3], NULL, 0 ), C = 1UL;
    if( !strcmp( argv[4], "geo" ) ) {
      if( argc != 8 ) return 2;
      unsigned long max_blob = strtoul( argv[5], NULL, 0 ), max_sigs = strtoul( argv[6], NULL, 0 ), m = strtoul( argv[7], NULL, 0 );
      fd_sha_long_geom_t g;
      if( fd_sha_long_geom( max_blob, max_sigs, 1UL, 1, &g ) ) return 2;
      if( fd_sha_long_geom( max_blob, max_sigs, m ? m : g.G, 1, &g ) ) return 2;
      C = g.C;
    }
    for( unsigned long sz=lo; sz<=hi; sz++ ) {
      uint8_t * msg = (uint8_t *)malloc( sz );               /* exactly sz bytes (malloc( 0 ): never read) */
      for( unsigned long i=0; i<sz; i++ ) msg[i] = (uint8_t)( ( i * 131UL + 7UL ) & 255UL );
      unsigned long nb = fd_sha_long_blocks( sz );
      uint64_t total = (uint64_t)nb * 128UL;
      if( fwrite( &total, 1, 8, stdout ) != 8 ) return 1;
      for( unsigned long b=0; b<nb; b+=C ) {
        unsigned long k = nb - b < C ? nb - b : C;
        uint8_t * piece = (uint8_t *)malloc( k * 128UL );    /* exactly the piece: a write past it is caught */
        memset( piece, 0xEE, k * 128UL );
        fd_sha_long_pack( piece, msg, sz, b * 128UL, k * 128UL );
        if( fwrite( piece, 1, k * 128UL, stdout ) != k * 128UL ) return 1;
        free( piece );
      }
      free( msg );
    }
    return 0;
  }
  fprintf( stderr, "usage: %s stream LO HI 128|geo [MAX_BLOB MAX_SIGS M] | tail SZ | geometry LO HI\n", argv[0] );
  return 2;
}
