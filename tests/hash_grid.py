"""The hash-path grid: a corpus, built at test time, that walks what carries
message bytes into SHA-512 (fd_sha_stage / fd_sha_fetch / fd_sha_words, the
wave pair of fd_k_front, fd_k_sha512_batch) through every message length and
start alignment where its byte-level edge logic changes.  A helper with no
tests in it: tests/test_hash_grid.py checks the corpus itself on the CPU,
tests/test_gpu_hash_paths.py runs it on the device.

Rows
  grid    one valid signature for every message length 0..401 and every start
          alignment 0..15 (mod 16) of the message: 6,432 rows.  Lengths 0..401
          give every residue of (64 + sz) mod 128 at 1-4 blocks (PRE = 64) and
          every residue of sz mod 128 at 1-4 blocks (PRE = 0)
  giant   24 valid signatures over 1233 .. 65537 bytes at alignments 1, 7, 14
  dead    400 rows that never reach the hash: S >= L (ERR_SIG), the
          reference's early accept, msg_off + msg_sz one byte past
          the blob, and a sum that wraps 32 bits (both ERR_ARG, the engine's
          own code: the reference takes pointers and checks nothing)
  flip    for 64 grid rows and every giant: copies with one message bit
          flipped at the bytes where a block, a fetch chunk or the message
          ends, and one copy a byte shorter (ERR_MSG all)

sig_off, pub_off and msg_off of a row sit at three different residues mod 16,
at least one byte apart, in a blob of random bytes: every neighbour of a
message is noise, never zeros.  Keys and signatures are the host signer's
(fd_ed25519_sign_batch).

Orders
  ragged  live rows in a fixed-seed permutation, so a wave of 64 mixes lengths,
          giants and dead rows
  sorted  live rows by length
Dead rows are spread evenly through both, and the last live row's message is
placed last: it ends exactly at blob_sz."""
import hashlib

import numpy as np

import firedancer_amd as fa
from conftest import P

L = 2**252 + 27742317777372353535851937790883648493

GRID, GIANT, DEAD_SIG, DEAD_Q1, DEAD_PAST, DEAD_WRAP = range(6)
N_LEN = 402
GIANT_LENS = (1233, 4095, 4096, 4097, 8191, 8193, 65535, 65537)
GIANT_ALIGNS = (1, 7, 14)
N_DEAD = 400
DEAD_MSG = (0, 77, 1232, 5000)      # message bytes that a dead S >= L / Q1 row points at
# the ragged permutation: the first seed at which test_hash_grid's conditions on
# the order hold (three block counts in every wave, a last live row of >= 16 bytes)
RAGGED_SEED = 0
FLIP_LENS = (1, 2, 16, 46, 47, 48, 63, 64, 65, 111, 112, 127, 128, 129, 174, 175, 176, 191, 192, 193, 239, 240,
             302, 303, 304, 319, 320, 321, 400, 401)


def nblk(sz, pre=64):
    """SHA-512 blocks of a pre-byte prefix and sz message bytes"""
    return (pre + np.asarray(sz, np.int64) + 17 + 127) >> 7


class Rows:
    """rows before packing: kind, sz, align (msg_off mod 16), sig[n,64], pub[n,32],
    src (offset of the message bytes in store), seed[n,32] (live rows), origin"""

    def __len__(self):
        return len(self.kind)

    def live(self):
        return self.kind <= GIANT

    def msg(self, i):
        return self.store[int(self.src[i]):int(self.src[i]) + int(self.sz[i])].tobytes()


class Pack:
    """a packed order: blob (exactly blob_sz bytes), desc, row (index into the Rows),
    kind, sz, align per descriptor"""

    def __len__(self):
        return len(self.desc)


def build_rows():
    rng = np.random.default_rng(20270)
    kind, sz, align = [], [], []
    for s in range(N_LEN):
        for a in range(16):
            kind.append(GRID), sz.append(s), align.append(a)
    for s in GIANT_LENS:
        for a in GIANT_ALIGNS:
            kind.append(GIANT), sz.append(s), align.append(a)
    for j in range(N_DEAD):
        k = DEAD_SIG + j % 4
        kind.append(k), align.append((j // 4) % 16)
        sz.append(DEAD_MSG[(j // 4) % 4] if k in (DEAD_SIG, DEAD_Q1) else 0)
    r = Rows()
    r.kind, r.sz, r.align = np.array(kind), np.array(sz, np.int64), np.array(align)
    n = len(r)
    r.src = np.cumsum(r.sz) - r.sz
    r.store = rng.integers(0, 256, int(r.sz.sum()), dtype=np.uint8)
    r.seed = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    r.sig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    r.pub = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    live = np.nonzero(r.live())[0]
    pub, sig = fa.sign_batch(r.seed[live], r.store, r.src[live].astype(np.uint64), r.sz[live].astype(np.uint32))
    r.sig[live], r.pub[live] = sig, pub
    r.sig[r.kind == DEAD_SIG, 63] = 0xff                    # S >= 2^255
    q1 = r.kind == DEAD_Q1
    r.sig[q1, 63] = 0x10                                    # fd_ed25519_user.c:379: s[31] == 0x10 and
    r.sig[q1, 50] |= 1                                      # a nonzero byte in s[16..30]
    r.origin = np.arange(n)
    return r


def order_of(rows, name):
    """row indices in the named order, dead rows spread evenly through it"""
    live, dead = np.nonzero(rows.live())[0], np.nonzero(~rows.live())[0]
    if name == "ragged":
        live = live[np.random.default_rng(RAGGED_SEED).permutation(len(live))]
    elif name == "sorted":
        live = live[np.argsort(rows.sz[live], kind="stable")]
    else:
        raise ValueError(name)
    n = len(live) + len(dead)
    out = np.full(n, -1, np.int64)
    if len(dead):
        out[(np.arange(len(dead)) * n) // len(dead)] = dead
    out[out < 0] = live
    return out


def _scatter(blob, dst, store, src, sz):
    """blob[dst_i .. +sz_i) = store[src_i .. +sz_i) for every i, without a Python loop"""
    sz = np.asarray(sz, np.int64)
    tot = int(sz.sum())
    if not tot:
        return
    within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(sz) - sz, sz)
    blob[np.repeat(np.asarray(dst, np.int64), sz) + within] = store[np.repeat(np.asarray(src, np.int64), sz) + within]


def pack(rows, order, seed=1):
    order = np.asarray(order, np.int64)
    n = len(order)
    live_at = np.nonzero(rows.live()[order])[0]
    place = list(range(n))
    if len(live_at):                                        # the last live row's bytes go last
        place.remove(int(live_at[-1]))
        place.append(int(live_at[-1]))
    so, po, mo = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    cur = 0
    nxt = lambda c, res: c + ((res - c) % 16)               # noqa: E731  first offset >= c at residue res
    for j in place:
        i = order[j]
        a = int(rows.align[i])
        so[j] = nxt(cur + 1, (a + 5) % 16)
        po[j] = nxt(so[j] + 65, (a + 11) % 16)
        cur = po[j] + 32
        if rows.kind[i] <= DEAD_Q1:
            mo[j] = nxt(cur + 1, a)
            cur = mo[j] + int(rows.sz[i])
    p = Pack()
    blob_sz = int(cur)
    p.blob = np.random.default_rng(seed).integers(0, 256, blob_sz, dtype=np.uint8)
    p.row, p.kind, p.sz, p.align = order, rows.kind[order], rows.sz[order].copy(), rows.align[order]
    p.blob[so[:, None] + np.arange(64)[None, :]] = rows.sig[order]
    p.blob[po[:, None] + np.arange(32)[None, :]] = rows.pub[order]
    has = p.kind <= DEAD_Q1
    _scatter(p.blob, mo[has], rows.store, rows.src[order][has], p.sz[has])
    msz = p.sz.copy()
    past, wrap = p.kind == DEAD_PAST, p.kind == DEAD_WRAP
    msz[past] = 100
    mo[past] = blob_sz - 99                                 # msg_off + msg_sz == blob_sz + 1
    msz[wrap] = 0x40
    mo[wrap] = 0xfffffff0                                   # a 32-bit sum would be 0x30
    p.desc = np.zeros(n, fa.DESC_DTYPE)
    p.desc["sig_off"], p.desc["pub_off"], p.desc["msg_off"], p.desc["msg_sz"] = so, po, mo, msz
    p.sig, p.pub = rows.sig[order], rows.pub[order]
    return p


def flip_positions(sz, align):
    """message bytes whose flip a wrong block, chunk or tail edge would miss"""
    if sz < 1:
        return []
    pos = {0, sz - 1, 63, 64}
    b = (sz + 63) // 128                                    # the last block edge inside the message
    if b >= 1:
        pos |= {128 * b - 65, 128 * b - 64}
    e = sz - 1 - ((align + sz - 1) % 16)                    # the last 16-byte aligned address in it (fd_sha_stage)
    if e >= 1:
        pos |= {e - 1, e}
    bl = (64 + sz - 1) // 128                               # fd_sha_fetch: 16-byte chunks from the dword floor
    mb = 128 * bl - 64 if bl else 0                         # of the last block's first message byte
    base = mb - ((align + mb) % 4)
    e = base + 16 * ((sz - 1 - base) // 16)
    if e >= 1 and e > base:
        pos |= {e - 1, e}
    return sorted(x for x in pos if 0 <= x < sz)


def build_flips(rows):
    """Rows of the flip copies (kind of the source row; origin: its index)"""
    lens = sorted(FLIP_LENS + tuple(x for x in range(5, 400, 7) if x not in FLIP_LENS)[:64 - len(FLIP_LENS)])
    assert len(set(lens)) == 64
    src_rows = [s * 16 + (5 * j) % 16 for j, s in enumerate(lens)] + list(np.nonzero(rows.kind == GIANT)[0])
    parts, origin, sz, what = [], [], [], []
    for i in src_rows:
        m = np.frombuffer(rows.msg(i), np.uint8)
        for x in flip_positions(len(m), int(rows.align[i])):
            c = m.copy()
            c[x] ^= 1 << (x % 8)
            parts.append(c), origin.append(i), sz.append(len(m)), what.append(x)
        parts.append(m[:-1]), origin.append(i), sz.append(len(m) - 1), what.append(-1)
    f = Rows()
    origin = np.array(origin)
    f.origin, f.what = origin, np.array(what)               # what: the flipped byte, -1 the shorter copy
    f.kind, f.align, f.sz = rows.kind[origin], rows.align[origin], np.array(sz, np.int64)
    f.sig, f.pub, f.seed = rows.sig[origin], rows.pub[origin], rows.seed[origin]
    f.store = np.concatenate(parts)
    f.src = np.cumsum(f.sz) - f.sz
    f.sources = src_rows
    return f


def expected(ref, p):
    """ref_verify_batch's code of every row; ERR_ARG, the engine's own, where the
    descriptor leaves the blob (the reference is never shown those)"""
    n = len(p)
    out_of = p.kind >= DEAD_PAST
    off = np.where(out_of, 0, p.desc["msg_off"]).astype(np.uint64)
    sz = np.where(out_of, 0, p.desc["msg_sz"]).astype(np.uint32)
    out = np.full(n, 99, np.int32)
    sig, pub = np.ascontiguousarray(p.sig), np.ascontiguousarray(p.pub)
    ref.ref_verify_batch(n, P(sig), P(pub), P(p.blob), P(off), P(sz), P(out), 8)
    out[out_of] = fa.ERR_ARG
    return out


def digests(p):
    """SHA-512(R || A || M) of every live row by hashlib, [n,64]; zeros on dead rows"""
    dig = np.zeros((len(p), 64), np.uint8)
    for j in np.nonzero(p.kind <= GIANT)[0]:
        o, s = int(p.desc["msg_off"][j]), int(p.desc["msg_sz"][j])
        h = hashlib.sha512(p.sig[j, :32].tobytes() + p.pub[j].tobytes() + p.blob[o:o + s].tobytes()).digest()
        dig[j] = np.frombuffer(h, np.uint8)
    return dig


class Grid:
    pass


_cache = {}


def grid(ref):
    """the corpus, built once per process: rows, ragged, sorted, flips (Packs with .exp)"""
    if "g" not in _cache:
        g = Grid()
        g.rows = build_rows()
        g.ragged = pack(g.rows, order_of(g.rows, "ragged"), seed=2)
        g.sorted = pack(g.rows, order_of(g.rows, "sorted"), seed=3)
        g.flip_rows = build_flips(g.rows)
        g.flips = pack(g.flip_rows, np.arange(len(g.flip_rows)), seed=4)
        for p in (g.ragged, g.sorted, g.flips):
            p.exp = expected(ref, p)
        _cache["g"] = g
    return _cache["g"]
