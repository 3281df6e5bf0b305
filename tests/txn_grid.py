"""The transaction grammar grid: a corpus, built at test time from fixed seeds,
that walks the wire parser (firedancer_amd/csrc/fd_txn_core.h: fd_txn_parse on
the host, fd_k_txn_parse / fd_k_txn_ring_front one lane per transaction on the
device) rule by rule.  A helper with no tests in it: tests/test_txn_grid.py
checks the corpus itself on the CPU against the reference build,
tests/test_gpu_txn_grid.py runs it on the device, and
tests/test_txn_core_sanitize.py feeds it to the stand-alone sanitizer program.

The wire format, restated from fd_txn_core.h (nothing here is taken from the
reference's source):

  u8 signature_cnt | signature_cnt x 64 B
  message: [0x80 | version, u8 signature_cnt]  (v0)   or   u8 signature_cnt  (legacy)
           u8 readonly_signed_cnt, u8 readonly_unsigned_cnt
           cu16 acct_addr_cnt, acct_addr_cnt x 32 B, 32 B blockhash
           cu16 instr_cnt, per instruction: u8 program_id, cu16 acct_cnt, acct_cnt x u8,
                                            cu16 data_sz, data_sz x u8
           v0 only: cu16 table count, per table: 32 B address, cu16 writable_cnt,
                                            writable_cnt x u8, cu16 readonly_cnt, readonly_cnt x u8

build() takes a structural description (spec()) and returns the message bytes
and the offset of every field; any count may be given a forced compact-u16
width or raw bytes (spec(enc={...})), so a count can claim more or less than
what follows it.  Accepted payloads are really signed: their first
signature_cnt account addresses are keys derived from seeds with
fd_ed25519_public_batch, their signatures fa.sign_batch's over the message.
A fixed-seed share of the accepted payloads (one in ten) then gets one bad
signature at a varying position: S set to the group order, or a bit of R
flipped (the two kinds of test_gpu_txn_ring.corrupt).  Account bytes,
blockhashes and instruction data come from a seeded generator.

Every case states its side: want == 0 (accepted), a FD_TXN_REJ_* line, or ANY
(rejected, the line left to the reference).  A boundary comes as a pair of
cases that differ only in the value in question.

Compact-u16 widths a count can have in an accepted payload (WIDTHS):
  acct_addr_cnt  1, 2     (at most 256)
  instr_cnt      1, 2, 3  (three bytes an instruction: 21,789 fit in 65,535 bytes)
  acct_cnt       1, 2, 3  (one byte an index: 65,364 fit)
  data_sz        1, 2, 3  (65,364 fit)
  table count    1, 2     (at most 254)
  writable_cnt   1, 2     (at most 256 - acct_addr_cnt <= 255)
  readonly_cnt   1, 2     (the same)

Families (Case.fam)
  a  every FD_TXN_REJ_* line: hand-made payloads, and MUTATORS (one structural
     change aimed at one line) applied to random rich transactions.  Line 79
     (no byte for signature_cnt) has a single payload, the empty one; it is in
     the grid twice.
  b  each of the seven counts at 0, 1, 127, 128, 255, 256, 16,383, 16,384, 32,768
     and the largest value that parses, or the reject pair where its limit is
     lower; the malformed forms of every width at every count
  c  accounts: acct_addr_cnt, the read-only counts, signature_cnt
  d  lookup tables: their number, their counts at the limit, totals of 255 / 256 /
     257 three ways
  e  program ids and account indices at total - 1 and total, in the static and
     in the lookup range; total == 256
  f  instruction counts and footprints (20; 256, 3,570, 4,096 and two more than
     each; past 65,535), payload sizes 65,534 / 65,535 / 65,536 two ways,
     trailing bytes, a missing table count
  g  fill: ordinary signed payloads of 1-12 signatures, random structure, from the
     minimal 134 bytes to about 2 KB

Orders: `shuffled` (a fixed-seed permutation: giants and rejects share waves)
and `sorted` (by size)."""
import ctypes

import numpy as np

import firedancer_amd as fa
from conftest import P
from firedancer_amd import txn

L_ORDER = (2**252 + 27742317777372353535851937790883648493).to_bytes(32, "little")
ANY = -1
LINES = (73, 79, 81, 82, 85, 91, 93, 96, 98, 100, 102, 105, 106, 107, 109, 110, 113, 115, 136, 137, 138, 139, 140,
         161, 162, 163, 166, 170, 171, 172, 173, 175, 176, 189, 191, 200, 202)      # the FD_TXN_REJ_* enum
COUNTS = ("nacct", "ninstr", "na", "nd", "nlut", "nw", "nr")
CU16_LINE = dict(nacct=105, ninstr=113, na=137, nd=139, nlut=161, nw=170, nr=172)
WIDTHS = dict(nacct=(1, 2), ninstr=(1, 2, 3), na=(1, 2, 3), nd=(1, 2, 3), nlut=(1, 2), nw=(1, 2), nr=(1, 2))
N_FILL = 1600
N_BASES = 24                       # random rich transactions each mutator is applied to
GIANT = 16384                      # a payload larger than this counts against the cap of 40
# 1 signature, 2 accounts, legacy: bytes around the instructions, and the largest counts that fit 65,535
OVERHEAD = 1 + 64 + 3 + 1 + 64 + 32
MAX_INSTR = (65535 - OVERHEAD - 3) // 3           # 21,789, exactly 65,535 bytes
MAX_IN_ONE = 65535 - OVERHEAD - 1 - 1 - 3 - 1     # 65,364: acct_cnt or data_sz of a lone instruction


def cu16(v, width=None):
    """compact-u16 of v: minimal, or at a forced width (a longer form than minimal is malformed)"""
    if width is None:
        width = 1 if v < 0x80 else 2 if v < 0x4000 else 3
    if width == 1:
        return bytes([v & 0xff])
    if width == 2:
        return bytes([v & 0x7f | 0x80, (v >> 7) & 0xff])
    return bytes([v & 0x7f | 0x80, (v >> 7) & 0x7f | 0x80, (v >> 14) & 0xff])


def cu16_width(v):
    return len(cu16(v))


_DEFAULT = dict(nsig=1, v0=False, ros=0, rou=0, nacct=None, instrs=(), luts=(), enc=None, trailing=b"",
                sig_byte=None, hdr_sig=None, ver=0x80)


def spec(**kw):
    """a structural description.  nsig signature blocks (sig_byte: another first byte);
    v0 or legacy (ver: the version byte, hdr_sig: another num_required_signatures);
    ros / rou the read-only counts; nacct account addresses (default nsig + 1);
    instrs [(program_id, index bytes, data size)]; luts [(writable_cnt, readonly_cnt)],
    None: the table count is missing; enc {count key: forced width or raw bytes} with keys
    'nacct', 'ninstr', ('na', j), ('nd', j), 'nlut', ('nw', j), ('nr', j); trailing bytes"""
    s = dict(_DEFAULT)
    s.update(kw)
    if s["nacct"] is None:
        s["nacct"] = s["nsig"] + 1
    s["enc"] = dict(s["enc"] or {})
    s["instrs"] = [(int(p), bytes(i), int(d)) for p, i, d in s["instrs"]]
    s["luts"] = None if s["luts"] is None else [(int(w), int(r)) for w, r in s["luts"]]
    return s


def total_of(s):
    return s["nacct"] + sum(w + r for w, r in (s["luts"] or ()) if s["v0"])


class Pool:
    """seeded random bytes by the slice"""

    def __init__(self, seed, n=1 << 21):
        self.b = np.random.default_rng(seed).bytes(n)
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.b):
            self.at = (self.at * 7 + 13) % 4099
        r = self.b[self.at:self.at + n]
        self.at += n + 1
        return r

    def below(self, n, bound):
        """n bytes, each < bound (<= 256)"""
        return bytes((np.frombuffer(self.take(n), np.uint8).astype(np.uint16) * bound >> 8).astype(np.uint8))


def build(s, pool, pubs=None):
    """-> (message bytes, marks): marks[key] the message offset of 'hdr', 'ros', 'rou',
    'nacct', 'accts', 'hash', 'ninstr', ('pid'|'na'|'idx'|'nd'|'data', j), 'nlut',
    ('addr'|'nw'|'widx'|'nr'|'ridx', j), 'trail'.  pubs[k]: signer k's key."""
    m, mk = bytearray(), {}

    def cnt(key, v):
        mk[key] = len(m)
        e = s["enc"].get(key)
        m.extend(e if isinstance(e, (bytes, bytearray)) else cu16(v, e))

    nsig = s["nsig"]
    mk["hdr"] = 0
    if s["v0"]:
        m.append(s["ver"])
    m.append(nsig if s["hdr_sig"] is None else s["hdr_sig"])
    mk["ros"] = len(m)
    m.append(s["ros"])
    mk["rou"] = len(m)
    m.append(s["rou"])
    cnt("nacct", s["nacct"])
    mk["accts"] = len(m)
    a = bytearray(pool.take(32 * s["nacct"]))
    k = min(nsig, s["nacct"])
    if pubs is not None and k:
        a[:32 * k] = pubs[:k].tobytes()
    m += a
    mk["hash"] = len(m)
    m += pool.take(32)
    cnt("ninstr", len(s["instrs"]))
    for j, (pid, idx, nd) in enumerate(s["instrs"]):
        mk["pid", j] = len(m)
        m.append(pid)
        cnt(("na", j), len(idx))
        mk["idx", j] = len(m)
        m += idx
        cnt(("nd", j), nd)
        mk["data", j] = len(m)
        m += pool.take(nd)
    if s["v0"] and s["luts"] is not None:
        cnt("nlut", len(s["luts"]))
        for j, (nw, nr) in enumerate(s["luts"]):
            mk["addr", j] = len(m)
            m += pool.take(32)
            cnt(("nw", j), nw)
            mk["widx", j] = len(m)
            m += pool.take(nw)
            cnt(("nr", j), nr)
            mk["ridx", j] = len(m)
            m += pool.take(nr)
    mk["trail"] = len(m)
    m += s["trailing"]
    return bytes(m), mk


class Case:
    """name, fam, want (0, a line, ANY), payload, nsig (signature blocks in it), signed,
    bad (None, or (position, 'S' | 'R'): the one corrupted signature), spec"""

    def __repr__(self):
        return f"<{self.fam} {self.name} want={self.want} sz={len(self.payload)}>"


def corrupt(p, pos, kind):
    """test_gpu_txn_ring.corrupt's two kinds: S = L (ERR_SIG), or a bit of R flipped"""
    p = bytearray(p)
    if kind == "S":
        p[1 + 64 * pos + 32:1 + 64 * pos + 64] = L_ORDER
    else:
        p[1 + 64 * pos + 2] ^= 0x10
    return bytes(p)


# ------------------------------------------------------------------ random structure

def random_spec(rng, pool, nsig, budget, rich=False, v0=None):
    """a valid transaction of nsig signatures with about `budget` bytes of instruction
    accounts and data.  rich: v0 (unless told), two tables and three instructions at
    least, every count nonzero, total < 200 (what the mutators need)"""
    if v0 is None:
        v0 = bool(rng.integers(2))
    rich = int(rich)
    extra = int(rng.integers(2 if rich else 0, 20))
    nacct = nsig + extra
    luts = []
    if v0:
        luts = [(int(rng.integers(rich, 7)), int(rng.integers(rich, 7))) for _ in range(int(rng.integers(2 * rich, 5)))]
    total = nacct + sum(w + r for w, r in luts)
    instrs = []
    if total >= 2:
        n = int(rng.integers(3 * rich, 9))
        for _ in range(n):
            share = int(rng.integers(0, budget // n + 1))
            na = int(rng.integers(2 * rich, 12)) if rng.integers(8) else int(rng.integers(128, 200))
            na = min(na, share) if not rich else na
            nd = max(share - na, 2 * rich)
            instrs.append((int(rng.integers(1, total)), pool.below(na, total), nd))
    return spec(nsig=nsig, v0=v0, ros=int(rng.integers(0, nsig)), rou=int(rng.integers(0, extra + 1)), nacct=nacct,
                instrs=instrs, luts=luts)


# ------------------------------------------------------------------ mutators (family a)
# each: (name, needs_v0 (None: either), fn(spec dict, rng) -> (changes, cut, want)); cut = (mark key, delta)
# truncates the payload at that field; a cut of ("sigs", d) is counted from the payload's byte 1

def _last(s, what):
    return len(s[what]) - 1


def _with_enc(s, key, e):
    enc = dict(s["enc"])
    enc[key] = e
    return dict(enc=enc)


def _mal(r):
    """a malformed compact-u16: second byte 0, third byte 0, 4 or 0xff"""
    lo, mid = int(r.integers(0x80, 0x100)), int(r.integers(0x80, 0x100))
    return (bytes([lo, 0]), bytes([lo, mid, 0]), bytes([lo, mid, 4]), bytes([lo, mid, int(r.integers(4, 0x100))]))[int(r.integers(4))]


def _set_instr(s, j, pid=None, idx=None):
    ins = list(s["instrs"])
    p, i, d = ins[j]
    ins[j] = (p if pid is None else pid, i if idx is None else idx, d)
    return dict(instrs=ins)


def _poke(idx, k, v):
    b = bytearray(idx)
    b[k] = v
    return bytes(b)


def _split_to(s, total):
    """tables appended so that the account total becomes `total`, no count past its own limit"""
    need, lim = total - total_of(s), 256 - s["nacct"]
    add = []
    while need > 0:
        w = min(need, lim)
        add.append((w, 0) if len(add) % 2 == 0 else (0, w))
        need -= w
    return dict(luts=list(s["luts"]) + add)


MUTATORS = [
    ("sig_byte_0", None, lambda s, r: (dict(sig_byte=0), None, 81)),
    ("sig_byte_high", None, lambda s, r: (dict(sig_byte=int(r.integers(128, 256))), None, 81)),
    ("cut_in_sigs", None, lambda s, r: ({}, ("sigs", int(r.integers(0, 64 * s["nsig"]))), 82)),
    ("cut_after_sigs", None, lambda s, r: ({}, ("hdr", 0), 85)),
    ("version", True, lambda s, r: (dict(ver=int(r.integers(0x81, 0x100))), None, 91)),
    ("v0_sigcnt_missing", True, lambda s, r: ({}, ("hdr", 1), 93)),
    ("v0_sigcnt_other", True, lambda s, r: (dict(hdr_sig=(s["nsig"] + int(r.integers(1, 256))) & 0xff), None, 93)),
    ("legacy_sigcnt_other", False, lambda s, r: (dict(hdr_sig=(s["nsig"] + int(r.integers(1, 128))) & 0x7f), None, 96)),
    ("cut_after_hdr", None, lambda s, r: ({}, ("ros", 0), 98)),
    ("ro_signed", None, lambda s, r: (dict(ros=int(r.integers(s["nsig"], 256))), None, 100)),
    ("cut_after_ro_signed", None, lambda s, r: ({}, ("rou", 0), 102)),
    ("nacct_malformed", None, lambda s, r: (_with_enc(s, "nacct", _mal(r)), None, 105)),
    ("nacct_below_nsig", None, lambda s, r: (_with_enc(s, "nacct", cu16(s["nsig"] - 1)), None, 106)),
    ("ro_unsigned", None, lambda s, r: (dict(rou=s["nacct"] - s["nsig"] + 1), None, 107)),
    ("cut_in_accts", None, lambda s, r: ({}, ("accts", int(r.integers(0, 32 * s["nacct"]))), 109)),
    ("cut_in_hash", None, lambda s, r: ({}, ("hash", int(r.integers(0, 32))), 110)),
    ("ninstr_malformed", None, lambda s, r: (_with_enc(s, "ninstr", _mal(r)), None, 113)),
    ("cut_after_ninstr", None, lambda s, r: ({}, ("ninstr", 1), 115)),
    # one more instruction than there is; the table section goes, so nothing is left to read as one
    ("ninstr_one_more", None, lambda s, r: (dict(luts=None, **_with_enc(s, "ninstr", cu16(len(s["instrs"]) + 1))), None, 136)),
    ("na_malformed", None, lambda s, r: (_with_enc(s, ("na", int(r.integers(len(s["instrs"])))), _mal(r)), None, 137)),
    # one index at least stays: with fewer than 3 bytes the instruction is refused before its counts are read (136)
    ("cut_in_idx", None, lambda s, r: ({}, (("idx", _last(s, "instrs")), int(r.integers(1, len(s["instrs"][-1][1])))), 138)),
    ("nd_malformed", None, lambda s, r: (_with_enc(s, ("nd", int(r.integers(len(s["instrs"])))), _mal(r)), None, 139)),
    ("cut_in_data", None, lambda s, r: ({}, (("data", _last(s, "instrs")), int(r.integers(s["instrs"][-1][2]))), 140)),
    ("nlut_missing", True, lambda s, r: (dict(luts=None), None, 161)),
    ("nlut_malformed", True, lambda s, r: (_with_enc(s, "nlut", _mal(r)), None, 161)),
    ("nlut_255", True, lambda s, r: (_with_enc(s, "nlut", cu16(int(r.integers(255, 16384)))), None, 162)),
    ("cut_after_nlut", True, lambda s, r: ({}, ("nlut", 1), 163)),
    ("cut_in_lut_addr", True, lambda s, r: ({}, (("addr", _last(s, "luts")), int(r.integers(1, 32))), ANY)),     # 163 or 166
    ("nw_malformed", True, lambda s, r: (_with_enc(s, ("nw", int(r.integers(len(s["luts"])))), _mal(r)), None, 170)),
    ("cut_in_widx", True, lambda s, r: ({}, (("widx", _last(s, "luts")), int(r.integers(s["luts"][-1][0]))), ANY)),  # 163 or 171
    ("nr_malformed", True, lambda s, r: (_with_enc(s, ("nr", int(r.integers(len(s["luts"])))), _mal(r)), None, 172)),
    ("cut_in_ridx", True, lambda s, r: ({}, (("ridx", _last(s, "luts")), int(r.integers(s["luts"][-1][1]))), 173)),
    ("nw_past_limit", True, lambda s, r: (dict(luts=list(s["luts"]) + [(257 - s["nacct"], 0)]), None, 175)),
    ("nr_past_limit", True, lambda s, r: (dict(luts=list(s["luts"]) + [(0, 257 - s["nacct"])]), None, 176)),
    ("trailing", None, lambda s, r: (dict(trailing=bytes(r.integers(0, 256, int(r.integers(1, 40)), dtype=np.uint8))), None, 189)),
    ("total_257", True, lambda s, r: (_split_to(s, 257), None, 191)),
    ("pid_0", None, lambda s, r: (_set_instr(s, int(r.integers(len(s["instrs"]))), pid=0), None, 200)),
    ("pid_total", None, lambda s, r: (_set_instr(s, int(r.integers(len(s["instrs"]))), pid=total_of(s)), None, 200)),
    ("idx_total", None, lambda s, r: (_idx_total(s, r), None, 202)),
]


def _idx_total(s, r):
    j = int(r.integers(len(s["instrs"])))
    idx = s["instrs"][j][1]
    return _set_instr(s, j, idx=_poke(idx, int(r.integers(len(idx))), int(r.integers(total_of(s), 256))))


# ------------------------------------------------------------------ the grid

class Grid:
    """cases, shuffled / sorted (index arrays into cases), n_signed"""

    def payloads(self, order):
        return [self.cases[i].payload for i in getattr(self, order)]


class _Builder:
    def __init__(self):
        self.rng = np.random.default_rng(20280)
        self.pool = Pool(20281)
        self.cases = []
        self.names = set()

    def add(self, fam, name, want, s=None, cut=None, raw=None):
        assert name not in self.names, name
        self.names.add(name)
        c = Case()
        c.fam, c.name, c.want, c.spec, c.cut, c.raw, c.bad = fam, name, want, s, cut, raw, None
        self.cases.append(c)
        return c

    # -- a: hand-made payloads for the lines the mutators reach through one structure only
    def family_a(self):
        A = lambda *a, **k: self.add("a", *a, **k)          # noqa: E731
        A("empty", 79, raw=b"")
        A("empty_again", 79, raw=b"")
        A("five_alone", 82, raw=b"\x05")
        A("one_and_63_bytes", 82, raw=b"\x01" + self.pool.take(63))
        A("byte_0x80", 81, raw=b"\x80")
        A("byte_0xff_and_more", 81, raw=b"\xff" + self.pool.take(300))
        A("70001_bytes", 73, raw=b"\x01" + self.pool.take(70000))
        two = [(1, b"\x00", 3), (1, b"", 0)]
        # the second instruction has nothing left: the first one's data took the bytes that 3 * instr_cnt asked for
        A("instr_left_legacy", 136, spec(nsig=1, nacct=2, instrs=two[:1], enc={"ninstr": cu16(2)}))
        A("instr_left_two_short", 136, spec(nsig=2, nacct=3, instrs=[(1, b"\x00\x01", 5), (2, b"", 0)]), cut=(("pid", 1), 2))
        # the second table has nothing left: the first one's indices took the bytes that 34 * count asked for
        A("lut_addr_left", 166, spec(nsig=1, nacct=2, v0=True, luts=[(20, 14)], enc={"nlut": cu16(2)}))
        A("lut_addr_left_31", 166, spec(nsig=1, nacct=2, v0=True, luts=[(40, 30), (0, 0)]), cut=(("addr", 1), 31))
        A("luts_left", 163, spec(nsig=1, nacct=2, v0=True, luts=[(1, 1)], enc={"nlut": cu16(2)}))
        A("lutw_left", 171, spec(nsig=1, nacct=2, v0=True, luts=[(5, 0)], enc={("nw", 0): cu16(9)}))
        A("lutr_left", 173, spec(nsig=1, nacct=2, v0=True, luts=[(5, 3)], enc={("nr", 0): cu16(4)}))
        A("instrs_left_claim", 115, spec(nsig=1, nacct=2, instrs=two, enc={"ninstr": cu16(4)}))
        A("iacct_left_claim", 138, spec(nsig=1, nacct=2, instrs=[(1, b"\x00\x01", 0)], enc={("na", 0): cu16(4)}))
        A("idata_left_claim", 140, spec(nsig=1, nacct=2, instrs=[(1, b"", 7)], enc={("nd", 0): cu16(8)}))
        A("accts_left_claim", 109, spec(nsig=1, nacct=2, enc={"nacct": cu16(5)}))
        A("hash_left_0", 110, spec(nsig=1, nacct=2), cut=("hash", 0))
        A("hash_left_31", 110, spec(nsig=3, nacct=3, v0=True), cut=("hash", 31))
        # the mutators, each on N_BASES random rich transactions
        for name, needs_v0, fn in MUTATORS:
            for k in range(N_BASES):
                nsig = 1 + (k * 5 + len(name)) % 6
                base = random_spec(self.rng, self.pool, nsig, int(self.rng.integers(0, 600)), rich=True, v0=needs_v0)
                ch, cut, want = fn(base, self.rng)
                s = dict(base)
                s.update(ch)
                A(f"{name}/{k}", want, spec(**s), cut=cut)

    # -- b: compact-u16
    def family_b(self):
        B = lambda *a, **k: self.add("b", *a, **k)          # noqa: E731
        one = [(1, b"\x00", 1)]
        # acct_addr_cnt: 1..256
        B("nacct=0", 106, spec(nsig=1, nacct=0))
        B("nacct=1", 0, spec(nsig=1, nacct=1))
        for v in (127, 128, 255, 256):
            B(f"nacct={v}", 0, spec(nsig=1, nacct=v, instrs=one))
        B("nacct=257", 106, spec(nsig=1, nacct=257, instrs=one))
        for v in (16383, 16384, 32768, 65535):
            B(f"nacct={v}_claimed", 106, spec(nsig=1, nacct=2, instrs=one, enc={"nacct": cu16(v)}))
        # instr_cnt: whatever fits
        for v in (0, 1, 127, 128, 255, 256, 16383, 16384, MAX_INSTR):
            B(f"ninstr={v}", 0, spec(nsig=1, nacct=2, instrs=[(1, b"", 0)] * v))
        B(f"ninstr={MAX_INSTR + 1}_claimed", 115, spec(nsig=1, nacct=2, instrs=[(1, b"", 0)] * MAX_INSTR, enc={"ninstr": cu16(MAX_INSTR + 1)}))
        B("ninstr=32768_claimed", 115, spec(nsig=1, nacct=2, instrs=[(1, b"", 0)] * 3, enc={"ninstr": cu16(32768)}))
        # acct_cnt and data_sz of a lone instruction
        for v in (0, 1, 127, 128, 255, 256, 16383, 16384, 32768, MAX_IN_ONE):
            B(f"na={v}", 0, spec(nsig=1, nacct=2, instrs=[(1, self.pool.below(v, 2), 0)]))
            B(f"nd={v}", 0, spec(nsig=1, nacct=2, instrs=[(1, b"", v)]))
        B("nd=49152", 0, spec(nsig=1, nacct=2, instrs=[(1, b"", 49152)]))                     # third byte 3
        # one index more than fits takes data_sz's byte for an index; two more are not there
        B(f"na={MAX_IN_ONE + 1}_claimed", 139, spec(nsig=1, nacct=2, instrs=[(1, self.pool.below(MAX_IN_ONE, 2), 0)],
                                                    enc={("na", 0): cu16(MAX_IN_ONE + 1)}))
        B(f"na={MAX_IN_ONE + 2}_claimed", 138, spec(nsig=1, nacct=2, instrs=[(1, self.pool.below(MAX_IN_ONE, 2), 0)],
                                                    enc={("na", 0): cu16(MAX_IN_ONE + 2)}))
        B(f"nd={MAX_IN_ONE + 1}_claimed", 140, spec(nsig=1, nacct=2, instrs=[(1, b"", MAX_IN_ONE)], enc={("nd", 0): cu16(MAX_IN_ONE + 1)}))
        # table count: 0..254
        for v in (0, 1, 127, 128, 254, 255, 256):
            B(f"nlut={v}", 0 if v <= 254 else 162, spec(nsig=1, nacct=2, v0=True, instrs=one, luts=[(1, 1)] * min(v, 2) + [(0, 0)] * max(v - 2, 0)))
        for v in (16383, 16384, 32768):
            B(f"nlut={v}_claimed", 162, spec(nsig=1, nacct=2, v0=True, instrs=one, luts=[(1, 1)] * 2, enc={"nlut": cu16(v)}))
        # writable_cnt, readonly_cnt: 0..255 beside one account
        for key, line, left in (("nw", 175, 171), ("nr", 176, 173)):
            lut = (lambda v: (v, 0)) if key == "nw" else (lambda v: (0, v))
            for v in (0, 1, 127, 128, 255):
                B(f"{key}={v}", 0, spec(nsig=1, nacct=1, v0=True, luts=[lut(v)]))
            for v in (256, 16383, 16384):
                B(f"{key}={v}", line, spec(nsig=1, nacct=1, v0=True, luts=[lut(v)]))
            B(f"{key}=32768_claimed", left, spec(nsig=1, nacct=1, v0=True, luts=[lut(3)], enc={(key, 0): cu16(32768)}))
        # malformed forms at every count: the rest of the payload is that of the accepted base
        base = dict(nsig=2, nacct=5, v0=True, instrs=[(1, b"\x00\x02\x07", 4)], luts=[(2, 1)])
        B("malformed_base", 0, spec(**base))
        forms = (("second_0", b"\x85\x00"), ("third_0", b"\x85\x81\x00"), ("third_4", b"\x80\x80\x04"), ("third_ff", b"\xff\xff\xff"))
        key_of = dict(nacct="nacct", ninstr="ninstr", na=("na", 0), nd=("nd", 0), nlut="nlut", nw=("nw", 0), nr=("nr", 0))
        # where the payload ends inside a count, a check in front of the count may see it first:
        # 3 bytes an instruction (115), 34 a table (163)
        cut_line = {("na", 1): 115, ("nw", 1): 163}
        for c in COUNTS:
            for fname, raw in forms:
                B(f"{c}_{fname}", CU16_LINE[c], spec(**base, enc={key_of[c]: raw}))
            for fname, raw, at in (("cut_1_of_2", b"\x85\x01", 1), ("cut_1_of_3", b"\x85\x81\x01", 1), ("cut_2_of_3", b"\x85\x81\x01", 2)):
                B(f"{c}_{fname}", cut_line.get((c, at), CU16_LINE[c]), spec(**base, enc={key_of[c]: raw}), cut=(key_of[c], at))

    # -- c: accounts
    def family_c(self):
        C = lambda *a, **k: self.add("c", *a, **k)          # noqa: E731
        C("nacct=nsig=3", 0, spec(nsig=3, nacct=3, instrs=[(2, b"\x00\x01\x02", 2)]))
        C("nacct=nsig-1", 106, spec(nsig=3, nacct=2, instrs=[(1, b"\x00\x01", 2)]))
        for v in (128, 255, 256, 257):
            C(f"nsig=4_nacct={v}", 0 if v <= 256 else 106, spec(nsig=4, nacct=v, v0=True, instrs=[(v - 1 & 0xff or 1, bytes([0, 127, min(v, 256) - 1]), 9)]))
        C("nsig+rou=nacct", 0, spec(nsig=3, nacct=9, rou=6, instrs=[(8, b"\x03", 0)]))
        C("nsig+rou=nacct+1", 107, spec(nsig=3, nacct=9, rou=7, instrs=[(8, b"\x03", 0)]))
        C("rou=255_nacct=256", 0, spec(nsig=1, nacct=256, rou=255))
        C("rou=255_nacct=255", 107, spec(nsig=1, nacct=255, rou=255))
        C("ros=nsig-1", 0, spec(nsig=5, nacct=7, ros=4, instrs=[(6, b"\x00\x04\x05", 1)]))
        C("ros=nsig", 100, spec(nsig=5, nacct=7, ros=5, instrs=[(6, b"\x00\x04\x05", 1)]))
        C("ros=0_nsig=1", 0, spec(nsig=1, nacct=1))
        C("ros=1_nsig=1", 100, spec(nsig=1, nacct=1, ros=1))
        for v in (1, 2, 63, 64, 65, 126, 127):
            C(f"nsig={v}", 0, spec(nsig=v, nacct=v + 1, v0=bool(v & 1), instrs=[(v, bytes([0, v - 1, v]), 3)]))
        C("nsig=128", 81, spec(nsig=128, nacct=129, v0=True, instrs=[(128, bytes([0, 127, 128]), 3)]))
        C("nsig=128_legacy", 81, spec(nsig=128, nacct=129, instrs=[(128, bytes([0, 127, 128]), 3)]))

    # -- d: lookup tables
    def family_d(self):
        D = lambda *a, **k: self.add("d", *a, **k)          # noqa: E731
        for v in (0, 1, 127, 128, 254, 255):
            luts = [(1, 0), (0, 1), (2, 2)][:v] + [(0, 0)] * max(v - 3, 0)
            tot = 3 + sum(w + r for w, r in luts)
            D(f"tables={v}", 0 if v <= 254 else 162, spec(nsig=2, nacct=3, v0=True, instrs=[(tot - 1, bytes([0, tot - 1]), 2)], luts=luts))
        for nacct in (1, 2, 128, 255):
            lim = 256 - nacct
            ins = [(255, bytes([0, 255]), 1)]
            D(f"nacct={nacct}_nw={lim}", 0, spec(nsig=1, nacct=nacct, v0=True, instrs=ins, luts=[(lim, 0)]))
            D(f"nacct={nacct}_nw={lim + 1}", 175, spec(nsig=1, nacct=nacct, v0=True, instrs=ins, luts=[(lim + 1, 0)]))
            D(f"nacct={nacct}_nr={lim}", 0, spec(nsig=1, nacct=nacct, v0=True, instrs=ins, luts=[(0, lim)]))
            D(f"nacct={nacct}_nr={lim + 1}", 176, spec(nsig=1, nacct=nacct, v0=True, instrs=ins, luts=[(0, lim + 1)]))
        # both counts past the limit: the writable one is checked first
        D("nw_and_nr_past_limit", 175, spec(nsig=1, nacct=128, v0=True, luts=[(129, 129)]))
        D("nr_past_limit_second_table", 176, spec(nsig=1, nacct=128, v0=True, luts=[(1, 1), (3, 129)]))
        for tot in (255, 256, 257):
            want = 0 if tot <= 256 else 191
            ins = [(254, bytes([0, 10, 254]), 2)]
            add = tot - 10
            D(f"total={tot}_one_table", want, spec(nsig=2, nacct=10, v0=True, instrs=ins, luts=[(add // 2, add - add // 2)]))
            D(f"total={tot}_tables_of_one", want, spec(nsig=2, nacct=10, v0=True, instrs=ins, luts=[(1, 0), (0, 1)] * (add // 2) + [(1, 0)] * (add & 1)))
            D(f"total={tot}_writable_only", want, spec(nsig=2, nacct=10, v0=True, instrs=ins, luts=[(200, 0), (add - 200, 0)]))
        D("adtl_writable=255", 0, spec(nsig=1, nacct=1, v0=True, instrs=[(255, bytes([0, 255]), 0)], luts=[(255, 0)]))
        D("adtl_writable=128+127", 0, spec(nsig=1, nacct=1, v0=True, instrs=[(255, bytes([0, 255]), 0)], luts=[(128, 0), (127, 0)]))
        D("adtl_writable=254_readonly=1", 0, spec(nsig=1, nacct=1, v0=True, instrs=[(255, bytes([0, 255]), 0)], luts=[(254, 1)]))

    # -- e: indices
    def family_e(self):
        E = lambda *a, **k: self.add("e", *a, **k)          # noqa: E731
        where = (("static", dict(nsig=2, nacct=6), 6), ("static_v0", dict(nsig=2, nacct=6, v0=True), 6),
                 ("lookup", dict(nsig=2, nacct=4, v0=True, luts=[(3, 2)]), 9))
        for tag, kw, tot in where:
            for pid in (0, 1, tot - 1, tot, 255):
                E(f"{tag}_pid={pid}", 0 if 1 <= pid < tot else 200, spec(**kw, instrs=[(pid, b"\x00\x01", 2)]))
            if tag == "lookup":
                E("lookup_pid=5_idx_4_8", 0, spec(**kw, instrs=[(5, b"\x04\x08\x03", 2)]))
            # an index of total - 1 / total: the first, a middle and the last of the first and the last instruction
            for which in (0, 2):
                for pos in (0, 2, 4):
                    for v in (tot - 1, tot):
                        ins = [(1, b"\x00\x01\x00\x01\x00", 1), (2, b"\x01", 0), (1, b"\x00\x01\x00\x01\x00", 3)]
                        ins[which] = (1, _poke(ins[which][1], pos, v), ins[which][2])
                        E(f"{tag}_instr{which}_idx{pos}={v}", 0 if v < tot else 202, spec(**kw, instrs=ins))
        every = bytes(range(256))
        E("total=256_static_every_index", 0, spec(nsig=2, nacct=256, instrs=[(255, every, 5), (1, every[::-1], 0)]))
        E("total=256_lookup_every_index", 0, spec(nsig=2, nacct=100, v0=True, instrs=[(255, every, 5), (128, every[::-1], 0)], luts=[(100, 50), (0, 6)]))
        E("total=255_static_index_255", 202, spec(nsig=2, nacct=255, instrs=[(254, every, 5)]))
        E("total=255_lookup_index_255", 202, spec(nsig=2, nacct=100, v0=True, instrs=[(254, every, 5)], luts=[(100, 50), (0, 5)]))
        E("total=255_static_pid_255", 200, spec(nsig=2, nacct=255, instrs=[(255, every[:255], 5)]))
        E("total=255_lookup_pid_255", 200, spec(nsig=2, nacct=100, v0=True, instrs=[(255, every[:255], 5)], luts=[(100, 50), (0, 5)]))

    # -- f: sizes and footprints
    def family_f(self):
        F = lambda *a, **k: self.add("f", *a, **k)          # noqa: E731
        mini = (1, b"", 0)
        for v in (0, 1, 23, 24, 355):
            F(f"ninstr={v}_legacy", 0, spec(nsig=1, nacct=2, instrs=[(1, b"\x00", 2)] * v))
        # footprint = 20 + 10 instr_cnt + 8 table count
        for fp, ni, nl in ((256, 22, 2), (258, 23, 1), (3570, 355, 0), (3570, 351, 5), (3572, 352, 4), (4096, 406, 2), (4098, 407, 1),
                           (28, 0, 1), (30, 1, 0)):
            assert 20 + 10 * ni + 8 * nl == fp
            F(f"footprint={fp}_{ni}_instrs_{nl}_tables", 0, spec(nsig=2, nacct=3, v0=True, instrs=[(2, b"\x01", 1)] * ni, luts=[(1, 0)] * nl))
        for v in (6552, 6553, 6600, 8000, 10000, 12000, 20000):
            F(f"ninstr={v}_footprint={20 + 10 * v}", 0, spec(nsig=1, nacct=2, instrs=[mini] * v))
        # 65,534 / 65,535 / 65,536 bytes: one huge data_sz, and many minimal instructions
        for sz in (65534, 65535, 65536):
            want = 0 if sz <= 65535 else 73
            F(f"{sz}_bytes_one_data_sz", want, spec(nsig=1, nacct=2, instrs=[(1, b"", MAX_IN_ONE + sz - 65535)]))
            F(f"{sz}_bytes_minimal_instrs", want, spec(nsig=1, nacct=2, instrs=[mini] * (MAX_INSTR - 2) + [(1, b"", sz - 65532)]))
        tables = cu16(2) + self.pool.take(32) + b"\x01\x05\x00" + self.pool.take(32) + b"\x00\x01\x06"
        F("v0_with_table_section", 0, spec(nsig=1, nacct=2, v0=True, instrs=[(1, b"\x00\x02", 2)], luts=[(1, 0), (0, 1)]))
        F("legacy_with_table_section", 189, spec(nsig=1, nacct=2, instrs=[(1, b"\x00\x01", 2)], trailing=tables))
        F("legacy_without_table_section", 0, spec(nsig=1, nacct=2, instrs=[(1, b"\x00\x01", 2)]))
        F("legacy_one_trailing_byte", 189, spec(nsig=1, nacct=2, instrs=[(1, b"\x00\x01", 2)], trailing=b"\x00"))
        F("v0_zero_tables", 0, spec(nsig=1, nacct=2, v0=True, instrs=[(1, b"\x00\x01", 2)]))
        F("v0_table_count_missing", 161, spec(nsig=1, nacct=2, v0=True, instrs=[(1, b"\x00\x01", 2)], luts=None))
        F("v0_trailing_after_tables", 189, spec(nsig=1, nacct=2, v0=True, instrs=[(1, b"\x00\x01", 2)], luts=[(1, 1)], trailing=b"\x01"))

    # -- g: fill
    def family_g(self):
        for k in range(N_FILL):
            nsig = 1 + int(self.rng.integers(12)) if k % 4 == 0 else 1 + int(self.rng.integers(3))
            if k % 100 == 0:
                s = spec(nsig=1 + (k // 100) % 12, nacct=1 + (k // 100) % 12)                                # minimal
            else:
                s = random_spec(self.rng, self.pool, nsig, max(0, int(self.rng.integers(-200, 1600 - 97 * nsig))))
            self.add("g", f"fill/{k}", 0, s)

    # -- assemble, sign, corrupt
    def finish(self):
        cases = self.cases
        n_keys = sum(c.spec["nsig"] for c in cases if c.want == 0)
        seeds = self.rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
        pubs = np.zeros((n_keys, 32), np.uint8)
        fa.lib().fd_ed25519_public_batch(n_keys, P(seeds), P(pubs), 8)
        at, msgs, who = 0, [], []
        for c in cases:
            c.signed = False
            if c.raw is not None:
                c.nsig, c.msg, c.marks = 0, None, {}
                continue
            k = c.spec["nsig"]
            c.nsig = k
            c.signed = c.want == 0
            c.keys = slice(at, at + k) if c.signed else None
            c.msg, c.marks = build(c.spec, self.pool, pubs[at:at + k] if c.signed else None)
            if c.signed:
                at += k
                msgs.append(c.msg)
                who.append(c)
        assert at == n_keys
        blob = np.frombuffer(b"".join(msgs), np.uint8)
        sz = np.array([len(m) for m in msgs], np.int64)
        off = np.cumsum(sz) - sz
        cnt = np.array([c.nsig for c in who])
        pub2, sig = fa.sign_batch(seeds, blob, np.repeat(off, cnt).astype(np.uint64), np.repeat(sz, cnt).astype(np.uint32))
        assert np.array_equal(pub2, pubs)
        for c in cases:
            if c.raw is not None:
                c.payload = c.raw
                continue
            first = c.spec["sig_byte"]
            sigs = sig[c.keys].tobytes() if c.signed else self.pool.take(64 * c.nsig)
            p = bytes([c.nsig & 0xff if first is None else first]) + sigs + c.msg
            if c.cut is not None:
                key, d = c.cut
                p = p[:1 + d] if key == "sigs" else p[:1 + 64 * c.nsig + c.marks[key] + d]
            c.payload = p
        # one in ten of the accepted payloads gets one bad signature
        acc = [c for c in cases if c.want == 0]
        pick = np.random.default_rng(20282).permutation(len(acc))[:len(acc) // 10]
        for n, i in enumerate(sorted(pick.tolist())):
            c = acc[i]
            c.bad = ((n * 5 + n // 3) % c.nsig, "SR"[n & 1])
            c.payload = corrupt(c.payload, *c.bad)
        g = Grid()
        g.cases, g.n_signed = cases, n_keys
        g.shuffled = np.random.default_rng(20283).permutation(len(cases))
        g.sorted = np.argsort(np.array([len(c.payload) for c in cases]), kind="stable")
        return g


_cache = {}


def grid():
    """the corpus, built once per process"""
    if "g" not in _cache:
        b = _Builder()
        for f in "abcdefg":
            getattr(b, "family_" + f)()
        _cache["g"] = b.finish()
    return _cache["g"]


def claims(p):
    """the slots a payload claims on the ring: its first byte where that is in [1, 127]"""
    return p[0] if p and 1 <= p[0] <= 127 else 0


class Ref:
    """ref_txn_parse on every case: fp[i], line[i], raw[i] (the descriptor, b'' if rejected)"""


def reference(ref, g):
    if "r" not in _cache:
        f = ref.ref_txn_parse
        f.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_void_p, ctypes.c_void_p]
        f.restype = ctypes.c_ulong
        out = ctypes.create_string_buffer(1 << 19)
        ctr = txn.Counters()
        r = Ref()
        n = len(g.cases)
        r.fp, r.line, r.raw = np.zeros(n, np.int64), np.zeros(n, np.int64), []
        for i, c in enumerate(g.cases):
            ctr.failure_cnt = 0
            r.fp[i] = f(c.payload, len(c.payload), out, ctypes.byref(ctr))
            r.line[i] = 0 if r.fp[i] else ctr.failure_ring[0]
            r.raw.append(out.raw[:r.fp[i]])
        _cache["r"] = r
    return _cache["r"]


def write_file(g, path):
    """every payload, each behind its length as a little-endian u32 (txn_core_harness's --grid)"""
    with open(path, "wb") as f:
        for c in g.cases:
            f.write(len(c.payload).to_bytes(4, "little"))
            f.write(c.payload)
