#ifndef HEADER_fd_txn_core_h
#define HEADER_fd_txn_core_h

/* fd_txn_core.h -- the Solana transaction wire parser as a small cursor
   machine that runs on the host (fd_txn_host.c wraps it into fd_txn_parse)
   and in a HIP kernel (fd_k_txn_parse, one lane per transaction).

   It restates the acceptance rules of the reference parser
   (src/ballet/txn/fd_txn_parse.c:7-217, compact-u16 rules
   src/ballet/txn/fd_compact_u16.h:20-90).  The descriptor it writes is
   byte-identical to the reference's fd_txn_t for every accepted payload,
   every rejected payload returns 0, and each rejection reason is the
   reference's source line for that check (FD_TXN_REJ_* below: the
   reference stores __LINE__ in its failure ring).

   static inline, C and C++, no libc.  Every byte is read through a bounds
   check against payload_sz first: nothing outside payload[0, payload_sz)
   is touched, whatever the bytes say. */

#include "fd_txn_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FD_TXN_CORE_FN static inline __host__ __device__
#else
#define FD_TXN_CORE_FN static inline
#endif

/* reference line of each check (fd_txn_parse.c) */
enum {
  FD_TXN_REJ_TOO_BIG      =  73,  /* payload_sz > 65535                          */
  FD_TXN_REJ_SIGCNT_LEFT  =  79,  /* no byte for signature_cnt                   */
  FD_TXN_REJ_SIGCNT       =  81,  /* signature_cnt not in [1,127]                */
  FD_TXN_REJ_SIGS_LEFT    =  82,  /* signatures truncated                        */
  FD_TXN_REJ_HDR_LEFT     =  85,  /* no message header byte                      */
  FD_TXN_REJ_VERSION      =  91,  /* versioned but not v0                        */
  FD_TXN_REJ_V0_SIGCNT    =  93,  /* v0: missing / mismatched num_required_sigs  */
  FD_TXN_REJ_LEG_SIGCNT   =  96,  /* legacy: header byte != signature_cnt        */
  FD_TXN_REJ_ROSIGNED_LEFT=  98,
  FD_TXN_REJ_ROSIGNED     = 100,  /* fee payer must be a writable signer         */
  FD_TXN_REJ_ROUNSIGNED_L = 102,
  FD_TXN_REJ_ACCTCNT_CU16 = 105,
  FD_TXN_REJ_ACCTCNT      = 106,
  FD_TXN_REJ_ACCTCNT_RO   = 107,
  FD_TXN_REJ_ACCTS_LEFT   = 109,
  FD_TXN_REJ_HASH_LEFT    = 110,
  FD_TXN_REJ_INSTRCNT_CU16= 113,
  FD_TXN_REJ_INSTRS_LEFT  = 115,
  FD_TXN_REJ_INSTR_LEFT   = 136,
  FD_TXN_REJ_IACCT_CU16   = 137,
  FD_TXN_REJ_IACCT_LEFT   = 138,
  FD_TXN_REJ_IDATA_CU16   = 139,
  FD_TXN_REJ_IDATA_LEFT   = 140,
  FD_TXN_REJ_LUTCNT_CU16  = 161,
  FD_TXN_REJ_LUTCNT       = 162,
  FD_TXN_REJ_LUTS_LEFT    = 163,
  FD_TXN_REJ_LUTADDR_LEFT = 166,
  FD_TXN_REJ_LUTW_CU16    = 170,
  FD_TXN_REJ_LUTW_LEFT    = 171,
  FD_TXN_REJ_LUTR_CU16    = 172,
  FD_TXN_REJ_LUTR_LEFT    = 173,
  FD_TXN_REJ_LUTW_CNT     = 175,
  FD_TXN_REJ_LUTR_CNT     = 176,
  FD_TXN_REJ_TRAILING     = 189,
  FD_TXN_REJ_TOTAL_ACCTS  = 191,
  FD_TXN_REJ_PROGRAM_ID   = 200,
  FD_TXN_REJ_ACCT_IDX     = 202
};

/* What every caller gets, with or without a descriptor buffer.  A rejected
   payload has footprint, sig_cnt, acct_addr_off and tag 0 and reject_line
   set; an accepted one reject_line 0.  version is FD_TXN_VLEGACY unless the
   payload parsed as v0. */
typedef struct {
  uint64_t tag;           /* first 8 bytes of signature 0, little-endian */
  uint32_t footprint;     /* fd_txn_parse's return value (past 65535 only for payloads far beyond the MTU) */
  uint16_t reject_line;   /* FD_TXN_REJ_* */
  uint16_t acct_addr_off; /* signer i's key is payload[acct_addr_off + 32 i ..) */
  uint8_t  sig_cnt;       /* signatures at payload[1 + 64 i ..), the message at payload[1 + 64 sig_cnt ..) */
  uint8_t  version;
} fd_txn_core_sum_t;

typedef struct {
  uint8_t const * p;
  unsigned long   sz;
  unsigned long   at;     /* invariant: at <= sz */
} fd_txn_cur_t;

FD_TXN_CORE_FN int fd_txn_cur_has( fd_txn_cur_t const * c, unsigned long n ) { return n <= c->sz - c->at; }

/* compact-u16: 1..3 little-endian 7-bit groups, minimal encoding only,
   third byte <= 3 (value < 2^16).  Returns the encoded width, 0 if
   malformed or not fully inside the payload. */
FD_TXN_CORE_FN unsigned long
fd_txn_cu16_read( fd_txn_cur_t const * c, uint16_t * out ) {
  uint8_t const * b = c->p + c->at;
  unsigned long   n = c->sz - c->at;
  if( n >= 1 && b[0] < 0x80 ) { *out = b[0]; return 1; }
  if( n >= 2 && b[1] < 0x80 ) {
    if( !b[1] ) return 0;
    *out = (uint16_t)((b[0] & 0x7f) | (b[1] << 7)); return 2;
  }
  if( n >= 3 && b[2] <= 3 ) {
    if( !b[2] ) return 0;
    *out = (uint16_t)((b[0] & 0x7f) | ((b[1] & 0x7f) << 7) | (b[2] << 14)); return 3;
  }
  return 0;
}

#define FD_TXN_REJECT_IF(cond, why) do { if( cond ) return (unsigned long)(why) << 32; } while(0)
#define FD_TXN_NEED(n, why)         FD_TXN_REJECT_IF( !fd_txn_cur_has( &c, (unsigned long)(n) ), (why) )
#define FD_TXN_CU16(var, why)       do { unsigned long w_ = fd_txn_cu16_read( &c, &(var) ); FD_TXN_REJECT_IF( !w_, (why) ); c.at += w_; } while(0)

/* One walk over the payload.  t != NULL: the descriptor is written as the
   walk goes (the caller vouches for fd_txn_footprint bytes at t, 2-byte
   aligned; a rejected payload leaves a partial descriptor there, as
   fd_txn_parse always has).  t == NULL: nothing is written.  Returns the
   footprint (< 2^32), or the rejection's FD_TXN_REJ_* line << 32.  The
   account-index checks re-read the instructions from the payload, so the
   walk never depends on what it wrote. */
FD_TXN_CORE_FN unsigned long
fd_txn_core_walk( uint8_t const * payload, unsigned long payload_sz, fd_txn_t * t, fd_txn_core_sum_t * sum ) {
  fd_txn_cur_t c;
  c.p = payload; c.sz = payload_sz; c.at = 0UL;
  FD_TXN_REJECT_IF( payload_sz > 0xffffUL, FD_TXN_REJ_TOO_BIG );

  /* signatures */
  FD_TXN_NEED( 1, FD_TXN_REJ_SIGCNT_LEFT );
  unsigned long nsig = payload[ c.at++ ];
  FD_TXN_REJECT_IF( nsig < 1 || nsig > FD_TXN_SIG_MAX, FD_TXN_REJ_SIGCNT );
  FD_TXN_NEED( FD_TXN_SIGNATURE_SZ*nsig, FD_TXN_REJ_SIGS_LEFT );
  unsigned long sig_off = c.at;
  c.at += FD_TXN_SIGNATURE_SZ*nsig;

  /* message header: optional version prefix, then the three counts */
  unsigned long msg_off = c.at;
  FD_TXN_NEED( 1, FD_TXN_REJ_HDR_LEFT );
  uint8_t h0 = payload[ c.at++ ];
  uint8_t version;
  if( h0 & 0x80 ) {
    version = (uint8_t)(h0 & 0x7f);
    FD_TXN_REJECT_IF( version != FD_TXN_V0, FD_TXN_REJ_VERSION );
    FD_TXN_NEED( 1, FD_TXN_REJ_V0_SIGCNT );
    FD_TXN_REJECT_IF( payload[ c.at ] != nsig, FD_TXN_REJ_V0_SIGCNT );
    c.at++;
  } else {
    version = FD_TXN_VLEGACY;
    FD_TXN_REJECT_IF( h0 != nsig, FD_TXN_REJ_LEG_SIGCNT );
  }
  FD_TXN_NEED( 1, FD_TXN_REJ_ROSIGNED_LEFT );
  uint8_t ro_signed = payload[ c.at++ ];
  FD_TXN_REJECT_IF( ro_signed >= nsig, FD_TXN_REJ_ROSIGNED );
  FD_TXN_NEED( 1, FD_TXN_REJ_ROUNSIGNED_L );
  uint8_t ro_unsigned = payload[ c.at++ ];

  /* static account addresses and blockhash */
  uint16_t nacct = 0;
  FD_TXN_CU16( nacct, FD_TXN_REJ_ACCTCNT_CU16 );
  FD_TXN_REJECT_IF( nacct < nsig || nacct > FD_TXN_ACCT_ADDR_MAX, FD_TXN_REJ_ACCTCNT );
  FD_TXN_REJECT_IF( nsig + ro_unsigned > nacct, FD_TXN_REJ_ACCTCNT_RO );
  FD_TXN_NEED( FD_TXN_ACCT_ADDR_SZ*nacct, FD_TXN_REJ_ACCTS_LEFT );
  unsigned long acct_off = c.at;
  c.at += FD_TXN_ACCT_ADDR_SZ*nacct;
  FD_TXN_NEED( FD_TXN_BLOCKHASH_SZ, FD_TXN_REJ_HASH_LEFT );
  unsigned long hash_off = c.at;
  c.at += FD_TXN_BLOCKHASH_SZ;

  /* instructions (each at least program id + two empty compact-u16s) */
  uint16_t ninstr = 0;
  FD_TXN_CU16( ninstr, FD_TXN_REJ_INSTRCNT_CU16 );
  FD_TXN_NEED( 3UL*ninstr, FD_TXN_REJ_INSTRS_LEFT );

  if( t ) {
    t->transaction_version   = version;
    t->signature_cnt         = (uint8_t)nsig;
    t->signature_off         = (uint16_t)sig_off;
    t->message_off           = (uint16_t)msg_off;
    t->readonly_signed_cnt   = ro_signed;
    t->readonly_unsigned_cnt = ro_unsigned;
    t->acct_addr_cnt         = nacct;
    t->acct_addr_off         = (uint16_t)acct_off;
    t->recent_blockhash_off  = (uint16_t)hash_off;
    t->instr_cnt             = ninstr;
  }

  unsigned long instr_at = c.at;
  for( unsigned long j=0; j<ninstr; j++ ) {
    FD_TXN_NEED( 3, FD_TXN_REJ_INSTR_LEFT );
    uint8_t pid = payload[ c.at++ ];
    uint16_t na = 0, nd = 0;
    FD_TXN_CU16( na, FD_TXN_REJ_IACCT_CU16 );
    FD_TXN_NEED( na, FD_TXN_REJ_IACCT_LEFT );
    unsigned long a_off = c.at; c.at += na;
    FD_TXN_CU16( nd, FD_TXN_REJ_IDATA_CU16 );
    FD_TXN_NEED( nd, FD_TXN_REJ_IDATA_LEFT );
    unsigned long d_off = c.at; c.at += nd;
    if( t ) {
      fd_txn_instr_t * ix = &t->instr[ j ];
      ix->program_id = pid; ix->_padding_reserved_1 = 0;
      ix->acct_cnt = na;    ix->data_sz = nd;
      ix->acct_off = (uint16_t)a_off; ix->data_off = (uint16_t)d_off;
    }
  }

  /* v0: address lookup tables (each at least 32 B address + two counts) */
  uint16_t nlut = 0;
  unsigned long lut_w = 0, lut_all = 0;
  if( version == FD_TXN_V0 ) {
    /* fd_txn_get_address_tables (a host-only inline of fd_txn_abi.h) */
    fd_txn_acct_addr_lut_t * lut = t ? (fd_txn_acct_addr_lut_t *)( t->instr + ninstr ) : (fd_txn_acct_addr_lut_t *)0;
    FD_TXN_CU16( nlut, FD_TXN_REJ_LUTCNT_CU16 );
    FD_TXN_REJECT_IF( nlut > FD_TXN_ADDR_TABLE_LOOKUP_MAX, FD_TXN_REJ_LUTCNT );
    FD_TXN_NEED( 34UL*nlut, FD_TXN_REJ_LUTS_LEFT );
    for( unsigned long j=0; j<nlut; j++ ) {
      FD_TXN_NEED( FD_TXN_ACCT_ADDR_SZ, FD_TXN_REJ_LUTADDR_LEFT );
      unsigned long addr = c.at; c.at += FD_TXN_ACCT_ADDR_SZ;
      uint16_t nw = 0, nr = 0;
      FD_TXN_CU16( nw, FD_TXN_REJ_LUTW_CU16 );
      FD_TXN_NEED( nw, FD_TXN_REJ_LUTW_LEFT );
      unsigned long w_off = c.at; c.at += nw;
      FD_TXN_CU16( nr, FD_TXN_REJ_LUTR_CU16 );
      FD_TXN_NEED( nr, FD_TXN_REJ_LUTR_LEFT );
      unsigned long r_off = c.at; c.at += nr;
      FD_TXN_REJECT_IF( nw > FD_TXN_ACCT_ADDR_MAX - nacct, FD_TXN_REJ_LUTW_CNT );
      FD_TXN_REJECT_IF( nr > FD_TXN_ACCT_ADDR_MAX - nacct, FD_TXN_REJ_LUTR_CNT );
      if( lut ) {
        lut[ j ].addr_off = (uint16_t)addr;
        lut[ j ].writable_cnt = (uint8_t)nw; lut[ j ].readonly_cnt = (uint8_t)nr;
        lut[ j ].writable_off = (uint16_t)w_off; lut[ j ].readonly_off = (uint16_t)r_off;
      }
      lut_w   += nw;
      lut_all += (unsigned long)nw + nr;
    }
  }
  FD_TXN_REJECT_IF( c.at != payload_sz, FD_TXN_REJ_TRAILING );
  unsigned long total = nacct + lut_all;
  FD_TXN_REJECT_IF( total > FD_TXN_ACCT_ADDR_MAX, FD_TXN_REJ_TOTAL_ACCTS );

  /* every account index must name an account; the program cannot be the
     fee payer (index 0).  The instructions were bounds-checked above, so
     this second pass over them cannot fail to decode. */
  c.at = instr_at;
  for( unsigned long j=0; j<ninstr; j++ ) {
    uint8_t pid = payload[ c.at++ ];
    uint16_t na = 0, nd = 0;
    c.at += fd_txn_cu16_read( &c, &na );
    FD_TXN_REJECT_IF( pid == 0 || pid >= total, FD_TXN_REJ_PROGRAM_ID );
    for( unsigned long k=0; k<na; k++ )
      FD_TXN_REJECT_IF( payload[ c.at + k ] >= total, FD_TXN_REJ_ACCT_IDX );
    c.at += na;
    c.at += fd_txn_cu16_read( &c, &nd );
    c.at += nd;
  }

  if( t ) {
    t->addr_table_lookup_cnt        = (uint8_t)nlut;
    t->addr_table_adtl_writable_cnt = (uint8_t)lut_w;
    t->addr_table_adtl_cnt          = (uint8_t)lut_all;
    t->_padding_reserved_1          = 0;
  }
  uint64_t tag = 0;
  for( int b=7; b>=0; b-- ) tag = (tag << 8) | payload[ sig_off + (unsigned long)b ];
  sum->tag           = tag;
  sum->acct_addr_off = (uint16_t)acct_off;
  sum->sig_cnt       = (uint8_t)nsig;
  sum->version       = version;
  /* fd_txn_footprint */
  return sizeof(fd_txn_t) + (unsigned long)ninstr*sizeof(fd_txn_instr_t) + (unsigned long)nlut*sizeof(fd_txn_acct_addr_lut_t);
}

#undef FD_TXN_REJECT_IF
#undef FD_TXN_NEED
#undef FD_TXN_CU16

/* out_cap value by which the caller vouches that out_buf takes any
   descriptor this payload can produce (fd_txn_parse's contract): the
   descriptor is written during a single walk */
#define FD_TXN_CORE_CAP_TRUSTED (~0UL)

/* Parse payload[0, payload_sz).  *sum is always filled.  out_buf (NULL, or
   out_cap bytes, 2-byte aligned) receives the fd_txn_t descriptor only if
   the payload parses and its footprint is at most out_cap; otherwise not a
   byte of it is written (the payload is walked once to decide, once more
   to write).  Returns the footprint, 0 if malformed. */
FD_TXN_CORE_FN unsigned long
fd_txn_core_parse( uint8_t const * payload, unsigned long payload_sz, void * out_buf, unsigned long out_cap,
                   fd_txn_core_sum_t * sum ) {
  int one_walk = out_buf && out_cap == FD_TXN_CORE_CAP_TRUSTED;
  sum->tag = 0; sum->footprint = 0; sum->reject_line = 0; sum->acct_addr_off = 0; sum->sig_cnt = 0;
  sum->version = FD_TXN_VLEGACY;
  unsigned long r = fd_txn_core_walk( payload, payload_sz, one_walk ? (fd_txn_t *)out_buf : (fd_txn_t *)0, sum );
  if( r >> 32 ) {
    sum->tag = 0; sum->acct_addr_off = 0; sum->sig_cnt = 0; sum->version = FD_TXN_VLEGACY;
    sum->reject_line = (uint16_t)(r >> 32);
    return 0UL;
  }
  sum->footprint = (uint32_t)r;
  if( !one_walk && out_buf && r <= out_cap ) (void)fd_txn_core_walk( payload, payload_sz, (fd_txn_t *)out_buf, sum );
  return r;
}

#endif /* HEADER_fd_txn_core_h */
