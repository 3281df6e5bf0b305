"""The corpora and the reading models of tests/test_gpu_stages.py, built and
checked on the CPU, so that a failure on the GPU is the device's:

- the point encodings of stage (a), with the number of encodings that are
  not on the curve counted by integer arithmetic (neither the reference nor
  the engine is asked);
- the scalars of stage (b) and the share of their rows the S range check
  leaves pending;
- the decode of an Ai table entry (stage c): the four lanes of entry e are
  the cached form [Z, Y-X, Y+X, 2d T] of (2e+1)(-A) (v_mul_d111 and
  v_subadd_12 on [Z, Y, X, T], the reference's avx/fd_ed25519_ge.c:423-481),
  validated against the reference's own double-scalar multiplication and
  shown to reject a wrong entry, swapped lanes and a wrong T lane.

CPU only."""
import hashlib

import numpy as np

from conftest import P, load_corpus
from firedancer_amd import corpus
from test_recode_host import edge_scalars

L = corpus.L
PRIME = corpus.P
SHIFTS = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)
INV2 = pow(2, PRIME - 2, PRIME)

E = sorted({s for s in edge_scalars() if s < L} | {2**252 + 1, L - 2})


def u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def fe_val(limbs):
    return sum(int(v) << sh for v, sh in zip(limbs, SHIFTS)) % PRIME


def fe_limbs(x):
    """x mod p as ten non-negative limbs of 26 / 25 bits"""
    x %= PRIME
    out = []
    for i, sh in enumerate(SHIFTS):
        w = 26 if i % 2 == 0 else 25
        out.append((x >> sh) & ((1 << w) - 1))
    return np.array(out, np.int32)


# ------------------------------------------------------------ (a) point encodings
def sqrt_branch(enc):
    """None: not on the curve; 0: the first root candidate fits; 1: it needs the
    factor sqrt(-1) (the second branch of the decompression)"""
    y = (int.from_bytes(enc, "little") & ((1 << 255) - 1)) % PRIME
    u, v = (y * y - 1) % PRIME, (corpus.D * y * y + 1) % PRIME
    x = u * pow(v, 3, PRIME) * pow(u * pow(v, 7, PRIME), (PRIME - 5) // 8, PRIME) % PRIME
    if (v * x * x - u) % PRIME == 0:
        return 0
    return 1 if (v * x * x + u) % PRIME == 0 else None


class Points:
    pass


def point_encodings():
    """the encodings stage (a) decompresses, in a fixed order, with what integer
    arithmetic says of each (Points.branch)"""
    rng = np.random.default_rng(4242)
    encs = []
    for name in ("adversarial", "small_order"):
        b, _ = load_corpus(name)
        for i in range(len(b)):
            encs += [b.pub(i), b.sig(i)[:32]]
    golden = len(set(encs))
    encs += corpus.small_order_encodings()
    encs += [corpus._enc(pt) for pt in corpus.torsion_points()]
    encs += corpus.off_curve_encodings(64, rng)
    # random keys: y at random until it is on the curve, either sign
    valid = []
    while len(valid) < 500:
        e = bytearray(rng.bytes(32))
        if sqrt_branch(bytes(e)) is not None and int.from_bytes(e, "little") & ((1 << 255) - 1) < PRIME:
            valid.append(bytes(e))
    encs += valid
    # y = 0, 1, p-1 and every non-canonical y (p .. p+18 = 2^255 - 1), with and without
    # bit 255; x = 0 with the sign bit set is y = 1, p-1, p+1 with it (the lax decoding
    # accepts it); off-curve y are among them and above
    edge = []
    for y in [0, 1, PRIME - 1] + [PRIME + j for j in range(19)]:
        for s in (0, 1):
            edge.append((y | (s << 255)).to_bytes(32, "little"))
    encs += edge
    seen, uniq = set(), []
    for e in encs:
        if e not in seen:
            seen.add(e)
            uniq.append(e)
    if len(uniq) % 2:
        uniq.append(uniq[0])
    c = Points()
    c.enc = uniq
    c.branch = [sqrt_branch(e) for e in uniq]
    c.counts = {"golden": golden, "valid": len(valid), "edge": len(edge), "small": len(corpus.small_order_encodings())}
    return c


def point_rows(c, seed=7):
    """rows (A, R) = consecutive encodings, S random below 2^252 (every row stays
    pending after the S check, so every front end decompresses both points), an
    eight-byte message: blob, desc, digests"""
    rng = np.random.default_rng(seed)
    import firedancer_amd as fa
    n = len(c.enc) // 2
    stride = 104
    blob = np.zeros(stride * n + 64, np.uint8)
    for i in range(n):
        S = int.from_bytes(rng.bytes(32), "little") >> 4
        blob[stride * i:stride * i + 96] = u8(c.enc[2 * i + 1] + S.to_bytes(32, "little") + c.enc[2 * i])
        blob[stride * i + 96:stride * i + 104] = u8(i.to_bytes(8, "little"))
    desc = np.zeros(n, fa.DESC_DTYPE)
    desc["sig_off"] = stride * np.arange(n)
    desc["pub_off"] = stride * np.arange(n) + 64
    desc["msg_off"] = stride * np.arange(n) + 96
    desc["msg_sz"] = 8
    dig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    return blob, desc, dig


def cover(total, sizes):
    """[lo, hi) windows that cover range(total): one of every length in sizes (largest
    first), then the largest again as often as it takes; a window that would pass the
    end is moved back to end there, so every length is one of sizes"""
    sizes = sorted(set(sizes), reverse=True)
    assert total >= sizes[0]
    out, lo, j = [], 0, 0
    while lo < total or j < len(sizes):
        n = sizes[j] if j < len(sizes) else sizes[0]
        j += 1
        lo = min(lo, total - n)
        out.append((lo, lo + n))
        lo += n
    return out


def test_cover():
    for total, sizes in ((1088, (1, 17)), (1088, (1, 63, 65, 257)), (65, (1, 31, 32, 33, 65)), (6077, (1, 255, 257))):
        w = cover(total, sizes)
        assert set(i for lo, hi in w for i in range(lo, hi)) == set(range(total))
        assert {hi - lo for lo, hi in w} == set(sizes), (total, sizes)
        assert len(w) <= len(sizes) + total // max(sizes) + 1


def test_point_corpus():
    c = point_encodings()
    n = len(c.enc)
    assert n % 2 == 0 and n // 2 >= 257 + 255 + 1
    rejected = sum(b is None for b in c.branch)
    # both square-root branches occur, and plenty of each
    assert sum(b == 0 for b in c.branch) > 200 and sum(b == 1 for b in c.branch) > 200
    # the corpus was built with at least the 64 generated off-curve encodings and the golden
    # corpora's off-curve cases
    assert rejected >= 64 + 2
    assert set(corpus.small_order_encodings()) <= set(c.enc) and c.counts["small"] == 14
    assert c.counts["valid"] == 500 and c.counts["edge"] == 44
    top = [e for e in c.enc if int.from_bytes(e, "little") & ((1 << 255) - 1) >= PRIME]
    assert len(top) == 38


# ------------------------------------------------------------ (b) scalars
def stream_scalars():
    """the E x E grid (S, k) and 512 random pairs, all below L"""
    rng = np.random.default_rng(515)
    pairs = [(S, k) for S in E for k in E]
    pairs += [(int.from_bytes(rng.bytes(32), "little") % L, int.from_bytes(rng.bytes(32), "little") % L) for _ in range(512)]
    return pairs


def s_pending(S):
    """fd_ed25519_user.c:372-393: does the S range check leave the signature pending"""
    s = S.to_bytes(32, "little")
    if s[31] > 0x10:
        return False
    if s[31] == 0x10:
        return not any(s[16:31]) and int.from_bytes(s[:16], "little") < L - 2**252
    return True


def stream_rows(pairs, pub, r_enc):
    """one row per pair: R = r_enc, A = pub (ordinary points), S the pair's, a message
    that differs per row.  -> blob, desc, dig (k as the 64-byte digest), khash (the k a
    real SHA-512 of R || A || M gives, mod L)"""
    import firedancer_amd as fa
    n = len(pairs)
    stride = 104
    blob = np.zeros(stride * n + 64, np.uint8)
    dig = np.zeros((n, 64), np.uint8)
    khash = []
    for i, (S, k) in enumerate(pairs):
        msg = (i ^ 0x5a5a5a5a).to_bytes(8, "little")
        blob[stride * i:stride * i + 104] = u8(r_enc + S.to_bytes(32, "little") + pub + msg)
        dig[i] = u8(k.to_bytes(64, "little"))
        khash.append(int.from_bytes(hashlib.sha512(r_enc + pub + msg).digest(), "little") % L)
    desc = np.zeros(n, fa.DESC_DTYPE)
    desc["sig_off"] = stride * np.arange(n)
    desc["pub_off"] = stride * np.arange(n) + 64
    desc["msg_off"] = stride * np.arange(n) + 96
    desc["msg_sz"] = 8
    return blob, desc, dig, khash


def test_stream_scalars_pending_share():
    pairs = stream_scalars()
    assert len(E) == 24 and len(pairs) == 24 * 24 + 512
    pend = [s_pending(S) for S, _ in pairs]
    assert all(S < L and k < L for S, k in pairs)
    assert sum(pend) == len(pairs)          # S < L throughout: every row is pending, well above the 90 % asked
    assert (0, 0) in pairs and any(2**252 <= S for S, _ in pairs)


# ------------------------------------------------------------ (c) the Ai table entry
def table_entry_fault(lanes, expect):
    """lanes: [4][12] raw dwords of one table entry; expect: the 30 limbs (X, Y, Z) of
    the reference's [2e+1](-A).  None if the entry is the cached form [Z, Y-X, Y+X,
    2d T] of a point projectively equal to it with both pad dwords 0, else what is off"""
    lanes = np.asarray(lanes)
    if lanes[:, 10:].any():
        return "pad dword set"
    l0, l1, l2, l3 = (fe_val(lanes[q, :10]) for q in range(4))
    Z, X, Y = l0, (l2 - l1) * INV2 % PRIME, (l2 + l1) * INV2 % PRIME
    Xe, Ye, Ze = (fe_val(expect[o:o + 10]) for o in (0, 10, 20))
    if Z == 0 or Ze == 0:
        return "Z = 0"
    if (X * Ze - Xe * Z) % PRIME:
        return "X / Z differs"
    if (Y * Ze - Ye * Z) % PRIME:
        return "Y / Z differs"
    if (l3 * Z - 2 * corpus.D * X * Y) % PRIME:
        return "lane 3 is not 2d X Y / Z"
    return None


def ref_neg_point(ref, enc):
    """the reference's decompression of enc with X and T negated (fd_ed25519_user.c:408-409)"""
    a = np.zeros(40, np.int32)
    b = np.zeros(40, np.int32)
    e = u8(enc)
    assert ref.ref_ge_frombytes_2(P(a), P(e), P(b), P(e)) == 0
    a[0:10] = -a[0:10]
    a[30:40] = -a[30:40]
    return a


def ref_table(ref, enc):
    """[8][30]: the reference's [2e+1](-A), e < 8, as p2 limbs (its DSM with b = 0)"""
    nega = ref_neg_point(ref, enc)
    out = np.zeros((8, 30), np.int32)
    zero = np.zeros(32, np.uint8)
    for e in range(8):
        o = np.zeros(30, np.int32)
        ref.ref_ge_dsm(P(o), P(u8((2 * e + 1).to_bytes(32, "little"))), P(nega), P(zero))
        out[e] = o
    return out


def model_entry(pt, e, z):
    """the cached form of (2e+1)(-pt) at projective scale z, as [4][12] dwords"""
    x, y = corpus._mul(2 * e + 1, ((PRIME - pt[0]) % PRIME, pt[1]))
    lanes = np.zeros((4, 12), np.int32)
    for q, v in enumerate((z, (y - x) * z, (y + x) * z, 2 * corpus.D * x * y * z)):
        lanes[q, :10] = fe_limbs(v)
    return lanes


def test_table_model_vs_reference(ref):
    rng = np.random.default_rng(99)
    keys = []
    while len(keys) < 6:
        e = bytes(rng.bytes(32))
        if int.from_bytes(e, "little") & ((1 << 255) - 1) < PRIME and corpus._dec(e) is not None:
            keys.append(e)
    for enc in keys:
        pt = corpus._dec(enc)
        exp = ref_table(ref, enc)
        for e in range(8):
            z = int.from_bytes(rng.bytes(32), "little") % PRIME or 1
            good = model_entry(pt, e, z)
            assert table_entry_fault(good, exp[e]) is None, (enc.hex(), e)
            # what the check must refuse
            assert table_entry_fault(model_entry(pt, (e + 1) % 8, z), exp[e]) is not None
            sw = good.copy()
            sw[[1, 2]] = sw[[2, 1]]
            assert table_entry_fault(sw, exp[e]) == "X / Z differs"
            t = good.copy()
            t[3, 0] ^= 1
            assert table_entry_fault(t, exp[e]) == "lane 3 is not 2d X Y / Z"
            p = good.copy()
            p[2, 11] = 1
            assert table_entry_fault(p, exp[e]) == "pad dword set"
            lz = good.copy()
            lz[0, 4] += 1
            assert table_entry_fault(lz, exp[e]) is not None
