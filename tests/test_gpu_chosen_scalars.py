"""Edge scalars through every DSM schedule, as VALID signatures.

Every other GPU parity test feeds the double-scalar multiplication a k that
is a SHA-512 output, so the device recoder (fd_ed25519_gpu_wnaf.h built for
gfx950: alignbit, LDS digit slots at stride 64, step-major and
signature-major op rows), fd_sc_reduce and the four DSM kernels only ever
see uniformly random 253-bit k, and a chosen S can only be part of a reject.
Engine.debug_verify_dig runs the product pipeline with the 64-byte digest
given by the caller, so k is ours: with a secret a, A = [a]B and
R = [S - k a mod L]B make [S]B - [k]A = R hold exactly, a valid signature at
any (S, k).  A wrong digit, table entry or step turns SUCCESS into ERR_MSG;
the negative controls (the same rows with k + 1) show the reverse.

The expected code of every row is composed from the reference's own
compiled functions (oracle/_ref/libfdref.so) along fd_ed25519_user.c:372-427
with the digest in place of the hash (ref_verify_dig), the corpus rows are
built at test time from the reference's scalar multiplication, and
test_chosen_digest_equals_hash_path pins the diagnostics entry to the
product path on the adversarial golden corpus.  test_edge_S_real_hash puts
the same edge values into S of really hashed signatures (no diagnostics
entry), through verify_packed and the ring.

Rows: 575 pairs (S, k) in E x E, E = the recoder's edge scalars below L;
1,835 structured and 2,048 random 512-bit digests for fd_sc_reduce; 575
negative controls.  Rows a6 and a7 of the DESIGN test table."""
import hashlib

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P, load_corpus, oracle_batch
from firedancer_amd import corpus
from test_recode_host import edge_scalars

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
PRIME = 2**255 - 19
SHIFTS = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)

E = sorted({s for s in edge_scalars() if s < L} | {2**252 + 1, L - 2})
SCHEDULES = ("uniform", "pooled", "quad", "oct")


def u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


# ------------------------------------------------------------ the reference side
def s_check(s):
    """fd_ed25519_user.c:372-393: the code the S range check settles, or None (pending)"""
    if s[31] > 0x10:
        return -1
    if s[31] == 0x10:
        if any(s[16:31]):
            return 0
        if int.from_bytes(s[:16], "little") >= L - 2**252:
            return -1
    return None


def ref_verify_dig(ref, dig, sig, pub):
    """fd_ed25519_verify (fd_ed25519_user.c:372-427, AVX build) from the reference's
    compiled functions, with `dig` in place of SHA-512(R || A || M)"""
    s = sig[32:]
    c = s_check(s)
    if c is not None:
        return c
    A = np.zeros(40, np.int32)
    R = np.zeros(40, np.int32)
    err = ref.ref_ge_frombytes_2(P(A), P(u8(pub)), P(R), P(u8(sig[:32])))
    if err:
        return err
    if ref.ref_ge_is_small_order(P(A)):
        return -2
    if ref.ref_ge_is_small_order(P(R)):
        return -1
    A[0:10] = -A[0:10]                      # fe_neg of X and T
    A[30:40] = -A[30:40]
    k = np.zeros(32, np.uint8)
    ref.ref_sc_reduce(P(u8(dig)), P(k))
    out = np.zeros(30, np.int32)
    ref.ref_ge_dsm(P(out), P(k), P(A), P(u8(s)))
    xz = np.zeros(10, np.int32)
    yz = np.zeros(10, np.int32)
    Z = np.ascontiguousarray(out[20:30])
    ref.ref_fe_mul_avx(P(xz), P(Z), P(np.ascontiguousarray(R[0:10])))
    ref.ref_fe_mul_avx(P(yz), P(Z), P(np.ascontiguousarray(R[10:20])))
    return 0 if (xz[:8] == out[0:8]).all() and (yz[:8] == out[10:18]).all() else -3


def ref_reduce(ref, dig):
    k = np.zeros(32, np.uint8)
    ref.ref_sc_reduce(P(u8(dig)), P(k))
    return k


def mul_base(ref, s, cache={}):
    """encoding of [s]B: the reference's DSM with a = 0 and the identity as A"""
    if s not in cache:
        ident = np.zeros(40, np.int32)
        ident[10] = ident[20] = 1
        out = np.zeros(30, np.int32)
        ref.ref_ge_dsm(P(out), P(np.zeros(32, np.uint8)), P(ident), P(u8(s.to_bytes(32, "little"))))
        X, Y, Z = (sum(int(v) << sh for v, sh in zip(out[o:o + 10], SHIFTS)) % PRIME for o in (0, 10, 20))
        zi = pow(Z, PRIME - 2, PRIME)
        x, y = X * zi % PRIME, Y * zi % PRIME
        cache[s] = (y | ((x & 1) << 255)).to_bytes(32, "little")
    return cache[s]


# ------------------------------------------------------------ the corpus
def limbs(vals):
    return sum(v << (21 * i) for i, v in enumerate(vals))


def reduction_digests(rng):
    """fd_sc_reduce inputs: multiples of L and their neighbours, powers of two and
    their predecessors, saturated / alternating / half 21-bit limbs, the ends of
    the range, and random 512-bit values"""
    top = 1 << 512
    d = [(L << j) + e for j in range(260) for e in (-1, 0, 1) if 0 <= (L << j) + e < top]
    d += [(1 << j) - 1 for j in range(1, 513)]
    d += [(1 << j) % top for j in range(1, 513)]
    d += [0x1FFFFF << (21 * i) for i in range(24)]
    d += [limbs([0x1FFFFF if (i + ph) & 1 else 0 for i in range(24)]) for ph in (0, 1)]
    d += [limbs([1 << 20] * 24), limbs([(1 << 20) - 1] * 24)]
    d += [top // L * L, top // L * L - 1, top - 1]
    structured = len(d)
    d += [int.from_bytes(rng.bytes(64), "little") for _ in range(2048)]
    assert all(0 <= x < top for x in d)
    return d, structured


PAIR, REDUCE, NEG = 0, 1, 2


class Chosen:
    pass


def build_chosen(ref):
    rng = np.random.default_rng(20261)
    # secret scalars: rows cycle over the first three (so the Ai tables differ); the
    # rest stand in where the reference rejects a valid row through a Q2 limb alias
    keys = [int.from_bytes(rng.bytes(32), "little") % L for _ in range(6)]
    assert len(set(keys)) == len(keys) and all(keys)
    pubs = [mul_base(ref, a) for a in keys]
    rows = []       # (family, sig, pub, digest, S, k)

    def valid_row(i, S, dig, kred):
        for j in (i % 3, 3, 4, 5):
            sig = mul_base(ref, (S - kred * keys[j]) % L) + S.to_bytes(32, "little")
            if ref_verify_dig(ref, dig, sig, pubs[j]) == 0:
                break
        return sig, pubs[j]     # the fixture asserts the reference's SUCCESS on it

    pairs = [(S, k) for S in E for k in E if (S, k) != (0, 0)]    # (0, 0): R would be the identity
    for i, (S, k) in enumerate(pairs):
        sig, pub = valid_row(i, S, k.to_bytes(64, "little"), k)
        rows.append((PAIR, sig, pub, k.to_bytes(64, "little"), S, k))
        rows.append((NEG, sig, pub, ((k + 1) % L).to_bytes(64, "little"), S, (k + 1) % L))
    digs, structured = reduction_digests(rng)
    for i, d in enumerate(digs):
        dig = d.to_bytes(64, "little")
        kred = int.from_bytes(ref_reduce(ref, dig).tobytes(), "little")
        assert kred == d % L, hex(d)                                  # the reference's own reduction is d mod L
        S = int.from_bytes(rng.bytes(32), "little") % L
        sig, pub = valid_row(i, S, dig, kred)
        rows.append((REDUCE, sig, pub, dig, S, kred))

    # shuffled with a fixed seed; the seed is the first at which pair rows fall on
    # every slot of a 128-slot pool (so on every lane of a quad and an oct group too)
    fam = np.array([r[0] for r in rows])
    for seed in range(100):
        perm = np.random.default_rng(seed).permutation(len(rows))
        if len(set((np.nonzero(fam[perm] == PAIR)[0] % 128).tolist())) == 128:
            break
    else:
        raise AssertionError("no shuffle puts pair rows on every pool slot")
    rows = [rows[i] for i in perm]
    c = Chosen()
    n = len(rows)
    c.family = fam[perm]
    c.blob = np.zeros(96 * n + 64, np.uint8)
    c.blob[:96 * n] = u8(b"".join(r[1] + r[2] for r in rows))
    c.desc = np.zeros(n, fa.DESC_DTYPE)
    c.desc["sig_off"] = 96 * np.arange(n)
    c.desc["pub_off"] = 96 * np.arange(n) + 64
    c.dig = u8(b"".join(r[3] for r in rows)).reshape(n, 64)
    c.S = [r[4] for r in rows]
    c.k = [r[5] for r in rows]
    c.exp = np.array([ref_verify_dig(ref, r[3], r[1], r[2]) for r in rows], np.int32)
    c.kref = np.stack([ref_reduce(ref, r[3]) for r in rows])
    c.counts = {"pair": len(pairs), "structured": structured, "random": len(digs) - structured}
    return c


@pytest.fixture(scope="module")
def chosen(ref):
    c = build_chosen(ref)
    assert len(E) == 24 and c.counts == {"pair": 575, "structured": 1835, "random": 2048}
    assert len(c.desc) <= 6000
    # conditions on the inputs: every constructed row is a valid signature by the
    # reference, every negative control a wrong one
    assert (c.exp[c.family != NEG] == fa.SUCCESS).all(), np.nonzero((c.exp != 0) & (c.family != NEG))[0][:10]
    assert (c.exp[c.family == NEG] == fa.ERR_MSG).all()
    for m in (8, 16, 128):
        assert len(set((np.nonzero(c.family == PAIR)[0] % m).tolist())) == m
    return c


@pytest.fixture(scope="module")
def eng():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    e = fa.Engine(0, 8192, 1 << 21)
    yield e
    e.close()


def set_schedule(e, name):
    """force one DSM schedule for every batch size used here (default: the product's knobs)"""
    e.dsm_pool_min, e.dsm_quad_max, e.dsm_oct_max = {
        "default": (262144, 32768, 64),
        "uniform": (1 << 62, 0, 0),
        "pooled": (0, 32768, 64),
        "quad": (262144, 32768, 0),
        "oct": (262144, 32768, 1 << 62)}[name]


@pytest.fixture
def sched(eng):
    yield lambda name: set_schedule(eng, name)
    set_schedule(eng, "default")
    eng.mode = fa.MODE_AVX


def mismatches(got, exp, c=None, lim=8):
    bad = np.nonzero(got != exp)[0]
    return [(int(i), int(exp[i]), int(got[i])) + ((int(c.family[i]), hex(c.S[i]), hex(c.k[i])) if c else ()) for i in bad[:lim]], len(bad)


# ------------------------------------------------------------ chosen digests
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_chosen_digest_codes(eng, sched, chosen, schedule):
    """the whole corpus in one call on each schedule: the reference composition's
    code on every row -- SUCCESS on the 575 pair and 3,883 reduction rows, ERR_MSG
    on the 575 negative controls (asserted on the inputs by the fixture)"""
    sched(schedule)
    codes, _, _ = eng.debug_verify_dig(chosen.blob, chosen.desc, chosen.dig)
    bad, nbad = mismatches(codes, chosen.exp, chosen)
    assert nbad == 0, (schedule, nbad, bad)
    assert (codes[chosen.family != NEG] == fa.SUCCESS).all() and (codes[chosen.family == NEG] == fa.ERR_MSG).all()


def test_chosen_digest_k(eng, sched, chosen, ref):
    """k_out is the reference's fd_ed25519_sc_reduce of the digest, byte for byte, on
    every pending row; status is 1 exactly where the reference gets past the S check
    (every row of the chosen corpus; the adversarial golden corpus has the others)"""
    sched("uniform")
    _, k, st = eng.debug_verify_dig(chosen.blob, chosen.desc, chosen.dig)
    assert (st == 1).all()
    bad = np.nonzero((k != chosen.kref).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), chosen.dig[i].tobytes().hex(), k[i].tobytes().hex()) for i in bad[:4]]
    b, _ = load_corpus("adversarial")
    dig = np.stack([u8(hashlib.sha512(b.sig(i)[:32] + b.pub(i) + b.msg(i)).digest()) for i in range(len(b))])
    for name in ("quad", "pooled"):       # signature-major and step-major prep
        sched(name)
        _, k, st = eng.debug_verify_dig(b.blob, b.desc, dig)
        pend = np.array([s_check(b.sig(i)[32:]) is None for i in range(len(b))])
        assert 0 < (~pend).sum() and ((st == 1) == pend).all()
        for i in range(len(b)):
            assert k[i].tobytes() == (ref_reduce(ref, dig[i]).tobytes() if pend[i] else bytes(32)), (name, i)


@pytest.mark.parametrize("n", [1, 7, 9, 17, 63, 65, 129, 257])
def test_chosen_digest_ragged(eng, sched, chosen, n):
    """prefixes of the shuffled corpus: partly filled oct / quad groups, blocks and
    pools (default knobs: oct up to 64 signatures, quad above; and the pooled DSM)"""
    for name in ("default", "pooled"):
        sched(name)
        codes, _, _ = eng.debug_verify_dig(chosen.blob, chosen.desc[:n], chosen.dig[:n])
        bad, nbad = mismatches(codes, chosen.exp[:n], chosen)
        assert nbad == 0, (name, n, bad)


def test_chosen_digest_modes(eng, sched, chosen):
    """portable and strict modes need no reference here: the encodings are canonical,
    the points of prime order, and neither mode has the AVX build's limb compare"""
    want = np.where(chosen.family == NEG, fa.ERR_MSG, fa.SUCCESS).astype(np.int32)
    for mode, names in ((fa.MODE_PORTABLE, ("uniform", "pooled")), (fa.MODE_STRICT, SCHEDULES)):
        eng.mode = mode
        for name in names:
            sched(name)
            codes, _, _ = eng.debug_verify_dig(chosen.blob, chosen.desc, chosen.dig)
            bad, nbad = mismatches(codes, want, chosen)
            assert nbad == 0, (mode, name, nbad, bad)


def test_chosen_digest_equals_hash_path(eng, sched):
    """with SHA-512(R || A || M) as the digest the entry is the product path: the
    adversarial golden corpus's recorded reference codes, invalid cases included"""
    b, expected = load_corpus("adversarial")
    dig = np.stack([u8(hashlib.sha512(b.sig(i)[:32] + b.pub(i) + b.msg(i)).digest()) for i in range(len(b))])
    assert len(set(b.label.tolist())) == len(corpus.CASES)
    for name in SCHEDULES + ("default",):
        sched(name)
        codes, _, _ = eng.debug_verify_dig(b.blob, b.desc, dig)
        bad, nbad = mismatches(codes, expected)
        assert nbad == 0, (name, nbad, bad)
        assert (eng.verify_packed(b.blob, b.desc) == expected).all(), name


def test_chosen_digest_args(eng, chosen):
    n = 16
    blob, desc, dig = chosen.blob, chosen.desc[:n].copy(), chosen.dig[:n]
    with pytest.raises(fa.EngineError):
        eng.debug_verify_dig(blob, desc, dig[:n - 1])                     # 64 bytes per signature
    with pytest.raises(fa.EngineError):
        eng.debug_verify_dig(blob, np.tile(desc, 1024), np.tile(dig, (1024, 1)))   # n > max_sigs
    with pytest.raises(fa.EngineError):
        eng.debug_verify_dig(np.zeros(eng.max_blob + 1, np.uint8), desc, dig)      # blob_sz > max_blob
    L_ = fa.lib()
    z = np.zeros(64 * n, np.uint8)
    for args in ((None, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(z), fa._p(z), None, None),
                 (eng._h, n, fa._p(blob), blob.nbytes, None, fa._p(z), fa._p(z), None, None),
                 (eng._h, n, fa._p(blob), blob.nbytes, fa._p(desc), None, fa._p(z), None, None),
                 (eng._h, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(z), None, None, None),
                 (eng._h, n, None, blob.nbytes, fa._p(desc), fa._p(z), fa._p(z), None, None)):
        assert L_.fd_ed25519_gpu_debug_verify_dig(*args) == fa.ERR_ARG
    # k_out and status_out may be NULL
    out = np.full(n, 99, np.int32)
    assert L_.fd_ed25519_gpu_debug_verify_dig(eng._h, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dig.copy()), fa._p(out), None, None) == 0
    assert (out == chosen.exp[:n]).all()
    codes, k, st = eng.debug_verify_dig(blob, desc[:0], dig[:0])
    assert codes.shape == (0,) and k.shape == (0, 32) and st.shape == (0,)
    # a descriptor outside the blob: ERR_ARG at that index only, no k
    desc["pub_off"][5] = blob.nbytes - 31
    desc["sig_off"][11] = 0xffffffc0
    codes, k, st = eng.debug_verify_dig(blob, desc, dig)
    exp = chosen.exp[:n].copy()
    exp[[5, 11]] = fa.ERR_ARG
    assert (codes == exp).all()
    assert (st[[5, 11]] == fa.ERR_ARG).all() and not k[[5, 11]].any() and (np.delete(st, [5, 11]) == 1).all()


# ------------------------------------------------------------ edge S, really hashed
def edge_s_batch(n, seed, off):
    """corpus.simple with S of every third row overwritten, cycling through E from E[off]"""
    b = corpus.simple(n, 64, seed)
    rows = np.arange(0, n, 3)
    vals = [E[(off + j) % len(E)] for j in range(len(rows))]
    for i, s in zip(rows, vals):
        o = int(b.desc["sig_off"][i]) + 32
        b.blob[o:o + 32] = u8(s.to_bytes(32, "little"))
    return b, rows, vals


@pytest.fixture(scope="module")
def edge_s(ref):
    """n = 24 and 32: the S-ahead wave of the latency front end runs (three batches
    each, so every value of E passes through it: S = 0 with no digits, its skip at
    s[31] = 0x10); n = 33 and 300: it does not"""
    out = []
    small = set()
    for n, off in ((24, 0), (24, 8), (24, 16), (32, 0), (32, 11), (32, 22), (33, 0), (300, 0)):
        b, rows, vals = edge_s_batch(n, 4000 + n + off, off)
        exp = oracle_batch(ref, b)
        # conditions on the inputs
        assert (np.delete(exp, rows) == fa.SUCCESS).all(), (n, off)
        if n <= 32:
            small |= set(vals)
        if n == 300:
            assert set(vals) == set(E)
        out.append((b, exp, rows, vals))
    assert small == set(E)
    assert any(2**252 <= s < L for s in E) and 0 in E
    return out


@pytest.mark.parametrize("schedule", SCHEDULES + ("default",))
def test_edge_S_real_hash(eng, sched, edge_s, schedule):
    """small, sparse and [2^252, L) values of S -- attacker-chosen bytes no corpus
    holds -- in really hashed signatures: the reference's code on every row"""
    sched(schedule)
    for b, exp, rows, vals in edge_s:
        got = eng.verify_packed(b.blob, b.desc)
        bad, nbad = mismatches(got, exp)
        assert nbad == 0, (schedule, len(b), bad, [hex(vals[list(rows).index(i)]) for i, _, _ in bad if i in rows])


def test_edge_S_real_hash_ring(eng, edge_s):
    """the same batches through submit / poll, two in flight"""
    for j in range(0, len(edge_s), 2):
        tickets = [(eng.submit(b.blob, b.desc), exp) for b, exp, _, _ in edge_s[j:j + 2]]
        for t, exp in tickets:
            out = np.full(len(exp), 99, np.int32)
            assert eng.poll(t, out)
            assert (out == exp).all(), len(exp)
