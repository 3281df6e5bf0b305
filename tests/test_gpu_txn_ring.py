"""Transactions through the pinned ring (include/fd_ed25519_gpu_txn.h:
fd_ed25519_gpu_submit_txns / _try_submit_txns / _poll_txns, the claimed-slot
layout, fd_k_txn_ring_front).

Expected values come from the reference build that travels with the tree, as
in tests/test_gpu_txn.py, whose `expect` is used as it is: ref_txn_parse says
which payloads parse, ref_verify_batch (libfdref_portable.so under
MODE_PORTABLE, the strict oracle under MODE_STRICT) gives each signature's
code.  Only the slot layout is restated here: on the ring sig_base is the
prefix of the claims (the first payload byte where it is in [1, 127]), an
unparsed transaction keeps the slots it claims, and their codes are
FD_ED25519_ERR_ARG.  Every batch is also held against Engine.verify_txns on
the same bytes.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P
from firedancer_amd import corpus, txn
from test_gpu_txn import expect, fixtures, ref_codes, refp, same  # noqa: F401  (refp: a fixture)

pytestmark = pytest.mark.gpu

MTU = corpus.TXN_MTU
POLL_KEEP = 2                      # FD_ED25519_GPU_POLL_KEEP
L_ORDER = (2**252 + 27742317777372353535851937790883648493).to_bytes(32, "little")
MAX_SIGS = 4096


# ---------------------------------------------------------------- expected values

def claims_of(blob, t):
    """the rule of the header, in Python"""
    c = np.zeros(len(t), np.int64)
    for i, (off, sz) in enumerate(zip(t["off"].tolist(), t["sz"].tolist())):
        if off + sz <= len(blob) and sz >= 1 and 1 <= blob[off] <= 127:
            c[i] = blob[off]
    return c


def ring_expect(ref, blob, t, codes_fn=None):
    """-> (results with sig_base the claim prefix, codes by claimed slot).  codes_fn:
    another build's per-signature codes of a corpus.Batch (default: the AVX reference)."""
    res, codes, descs, _ = expect(ref, blob, t)
    if codes_fn is not None and len(descs):
        codes = codes_fn(corpus.Batch(blob, descs))
        for i in np.nonzero(res["sig_cnt"])[0]:
            c = codes[res["sig_base"][i]:res["sig_base"][i] + res["sig_cnt"][i]]
            nz = np.nonzero(c)[0]
            res["status"][i] = c[nz[0]] if len(nz) else 0
    claim = claims_of(blob, t)
    base = np.cumsum(claim) - claim
    parsed = res["sig_cnt"] > 0
    assert np.array_equal(res["sig_cnt"][parsed], claim[parsed])          # a parsed payload has the count it claims
    ring = np.full(int(claim.sum()), fa.ERR_ARG, np.int32)
    for i in np.nonzero(parsed)[0]:
        ring[base[i]:base[i] + claim[i]] = codes[res["sig_base"][i]:res["sig_base"][i] + claim[i]]
    res["sig_base"] = base
    return res, ring


def ring_run(eng, blob, t):
    ticket = eng.submit_txns(blob, t)
    return eng.poll_txns(ticket, len(t), want_codes=True)


def check(eng, ref, blob, t, codes_fn=None, packed=True):
    exp, ecodes = ring_expect(ref, blob, t, codes_fn)
    got, codes = ring_run(eng, blob, t)
    same(got, exp)
    assert np.array_equal(codes, ecodes)
    if packed:
        # the synchronous call on the same bytes: every field but sig_base, and each
        # parsed transaction's codes
        pres, pcodes, _ = eng.verify_txns(blob, t, want_codes=True)
        for f in ("status", "tag", "footprint", "reject_line", "sig_cnt", "version"):
            assert np.array_equal(got[f], pres[f]), f
        for i in np.nonzero(got["sig_cnt"])[0]:
            k = int(got["sig_cnt"][i])
            assert np.array_equal(codes[got["sig_base"][i]:got["sig_base"][i] + k], pcodes[pres["sig_base"][i]:pres["sig_base"][i] + k])
    return got, codes


# ---------------------------------------------------------------- corpora

@pytest.fixture(scope="module")
def txns12():
    """about 1,100 transactions of 1..12 signatures (C2 shape, all valid)"""
    b = corpus.solana_txns(7200, seed=41, sig_dist=[1 / 12] * 12, max_sigs_per_txn=12)
    n = (len(b.blob) - 64) // MTU
    assert n >= 900
    return [bytes(b.blob[i * MTU:(i + 1) * MTU]) for i in range(n)]


@pytest.fixture(scope="module")
def big127():
    """one valid transaction of 127 signatures (far past the MTU), signed by the host signer"""
    k = 127
    rng = np.random.default_rng(6)
    seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    pub = np.zeros((k, 32), np.uint8)
    fa.lib().fd_ed25519_public_batch(k, P(seeds), P(pub), 4)
    msg = bytes([k, 0, 1, 0x80, 0x01]) + pub.tobytes() + bytes(rng.integers(0, 256, 32, dtype=np.uint8)) * 2 + bytes([1, k, 0, 0])
    body = np.frombuffer(msg, np.uint8).copy()
    _, sig = fa.sign_batch(seeds, body, np.zeros(k, np.uint64), np.full(k, len(msg), np.uint32))
    p = bytes([k]) + sig.tobytes() + msg
    assert txn.parse(p)["signature_cnt"] == 127
    return p


@pytest.fixture(scope="module")
def ring():
    e = fa.Engine(0, MAX_SIGS, 1 << 20, depth=3)
    yield e
    e.close()


def unparsed_claim(p):
    """truncated after the signatures: claims its slots, does not parse"""
    return p[:1 + 64 * p[0]]


def corrupt(p, a=None, b=None):
    """S of signature a set to L (ERR_SIG), a bit of R of signature b flipped"""
    p = bytearray(p)
    if a is not None:
        p[1 + 64 * a + 32:1 + 64 * a + 64] = L_ORDER
    if b is not None:
        p[1 + 64 * b + 2] ^= 0x10
    return bytes(p)


# ---------------------------------------------------------------- 1. block edges

@pytest.mark.parametrize("n_txn", [1, 255, 256, 257, 513])
def test_block_edges(ring, ref, txns12, big127, n_txn):
    """transactions 0, 255, 256 and the last claim slots and do not parse; first bytes 0 and
    0x80, an empty and an out-of-bounds entry; a 127-signature transaction whose slots lie
    across two rounds of its block's slot walk; a bad second signature before a bad sixth"""
    ps = list(txns12[:n_txn])
    if n_txn == 1:
        blob, t = txn.pack(ps, gap=3, first=1)
        got, _ = check(ring, ref, blob, t)                        # the lone valid transaction
        assert got["status"][0] == 0 and got["sig_cnt"][0] == ps[0][0]
    spoiled = [w for w in (0, 255, 256, n_txn - 1) if w < n_txn]
    for w in spoiled:
        ps[w] = unparsed_claim(ps[w])
    oob = None
    if n_txn >= 255:
        ps[3] = b"\x00" + ps[3][1:]
        ps[5] = b"\x80" + ps[5][1:]
        ps[7] = b""
        oob = 9
        twelve = next(p for p in txns12[600:] if p[0] == 12)
        ps[11] = corrupt(twelve, a=5, b=1)
        # the 127 slots start 150..250 slots past a multiple of 256 from the block's first
        # slot: the last lanes of one round and the first of the next write them
        claim = np.array([p[0] if p and 1 <= p[0] <= 127 else 0 for p in ps])
        claim[oob] = 0
        base = np.cumsum(claim) - claim
        at = next(i for i in range(20, 250) if 150 <= base[i] % 256 <= 250)
        ps[at] = big127
    blob, t = txn.pack(ps, gap=3, first=1)
    if oob is not None:
        t[oob] = (len(blob) - 10, 11)                             # one byte past the end
    assert (t["off"] & 1).any() and int(claims_of(blob, t).sum()) <= MAX_SIGS
    got, codes = check(ring, ref, blob, t)
    for w in spoiled:
        assert got["status"][w] == fa.ERR_TXN and got["reject_line"][w] == 85 and got["sig_cnt"][w] == 0
        k = t["sz"][w] // 64
        assert k >= 1 and (codes[got["sig_base"][w]:got["sig_base"][w] + k] == fa.ERR_ARG).all()
        if w + 1 < n_txn:
            assert got["sig_base"][w + 1] == got["sig_base"][w] + k     # it kept its slots
    if n_txn >= 255:
        assert got["status"][[3, 5, 7, 9]].tolist() == [fa.ERR_TXN, fa.ERR_TXN, fa.ERR_TXN, fa.ERR_ARG]
        assert got["reject_line"][[3, 5, 7, 9]].tolist() == [81, 81, 79, 0]
        assert got["sig_base"][4] == got["sig_base"][3] and got["sig_base"][10] == got["sig_base"][9]
        b11 = got["sig_base"][11]
        assert codes[b11 + 5] == fa.ERR_SIG and codes[b11 + 1] not in (0, fa.ERR_SIG) and got["status"][11] == codes[b11 + 1]
        assert got["sig_cnt"][at] == 127 and got["status"][at] == 0
        lo = got["sig_base"][0]
        assert (got["sig_base"][at] - lo) // 256 != (got["sig_base"][at] + 126 - lo) // 256


def test_nothing_claims_anything(ring, ref):
    """a valid batch: the front kernel alone, every status ERR_TXN or ERR_ARG"""
    ps = [b"", b"\x00" * 40, b"\x80" + b"\x01" * 100, b"\xff"]
    blob, t = txn.pack(ps, gap=1, first=1)
    t = np.concatenate([t, np.array([(len(blob), 1), (0xFFFFFFFF, 0xFFFFFFFF)], fa.TXN_DTYPE)])
    got, codes = check(ring, ref, blob, t)
    assert len(codes) == 0 and got["status"].tolist() == [fa.ERR_TXN] * 4 + [fa.ERR_ARG] * 2 and not got["sig_base"].any()


# ---------------------------------------------------------------- 2. capacity

def exactly(txns12, total):
    """a prefix of the corpus topped up with one-signature transactions to claim `total`"""
    ps, s = [], 0
    for p in txns12:
        if s + p[0] > total - 12:
            break
        ps.append(p)
        s += p[0]
    ones = [p for p in txns12 if p[0] == 1]
    while s < total:
        ps.append(ones[(total - s) % len(ones)])
        s += 1
    return ps


def test_capacity(ring, ref, txns12):
    L = fa.lib()
    ps = exactly(txns12, MAX_SIGS)
    blob, t = txn.pack(ps, gap=0, first=0)
    assert fa.txn_claims(blob, t)[1] == MAX_SIGS
    got, codes = check(ring, ref, blob, t, packed=False)
    assert len(codes) == MAX_SIGS and not got["status"].any()
    over = ps + [next(p for p in txns12 if p[0] == 1)]
    blob1, t1 = txn.pack(over, gap=0, first=0)
    assert fa.txn_claims(blob1, t1)[1] == MAX_SIGS + 1
    ticket = ctypes.c_ulong(0)
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, len(t1), P(blob1), blob1.nbytes, P(t1), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_submit_txns(ring._h, len(t1), P(blob1), blob1.nbytes, P(t1), ctypes.byref(ticket)) == fa.ERR_ARG
    assert ticket.value == 0
    # the other limits: nothing queued either
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, 0, P(blob), blob.nbytes, P(t), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, MAX_SIGS + 1, P(blob), blob.nbytes, P(t), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, len(t), P(blob), ring.max_blob + 1, P(t), ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, len(t), P(blob), blob.nbytes, None, ctypes.byref(ticket)) == fa.ERR_ARG
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, len(t), P(blob), blob.nbytes, P(t), None) == fa.ERR_ARG
    # no slot was lost: depth further submissions all succeed
    sb, st = txn.pack(txns12[:5], gap=1, first=1)
    tickets = [ring.submit_txns(sb, st) for _ in range(ring.depth)]
    exp, ecodes = ring_expect(ref, sb, st)
    for k in tickets:
        res, codes = ring.poll_txns(k, len(st), want_codes=True)
        same(res, exp)
        assert np.array_equal(codes, ecodes)
    assert L.fd_ed25519_gpu_poll_txns(ring._h, tickets[0], P(np.zeros(5, fa.TXN_RESULT_DTYPE)), None, 1) == fa.ERR_ARG   # collected
    assert L.fd_ed25519_gpu_poll_txns(ring._h, 1 << 40, None, None, 1) == fa.ERR_ARG                                  # NULL res


# ---------------------------------------------------------------- 3. the ring itself

def mixed(txns12, lo, hi, bad):
    ps = list(txns12[lo:hi])
    for w in bad:
        ps[w] = corrupt(ps[w], b=ps[w][0] - 1)
    ps[1] = unparsed_claim(ps[1])
    return txn.pack(ps, gap=1, first=1)


def test_ring_of_three(ring, ref, txns12):
    """three different batches in flight, a full ring, out-of-order polls, a resubmission:
    each ticket's results are its own (they would not be if slots shared scratch)"""
    L = fa.lib()
    assert ring.depth == 3
    batches = [mixed(txns12, 0, 300, [5, 100]), mixed(txns12, 300, 420, [7]), mixed(txns12, 420, 700, [0, 200, 279]),
               mixed(txns12, 700, 760, [33])]
    exps = [ring_expect(ref, b, t) for b, t in batches]
    assert len({len(e[1]) for e in exps}) == 4 and len({tuple(e[0]["status"].tolist()) for e in exps}) == 4
    tk = [ring.submit_txns(b, t) for b, t in batches[:3]]
    assert tk[0] < tk[1] < tk[2]
    b3, t3 = batches[3]
    assert ring.try_submit_txns(b3, t3) is None
    ticket = ctypes.c_ulong(0)
    assert L.fd_ed25519_gpu_try_submit_txns(ring._h, len(t3), P(b3), b3.nbytes, P(t3), ctypes.byref(ticket)) == 0
    assert L.fd_ed25519_gpu_submit_txns(ring._h, len(t3), P(b3), b3.nbytes, P(t3), ctypes.byref(ticket)) == fa.ERR_ARG
    with pytest.raises(fa.EngineError):
        ring.submit_txns(b3, t3)

    def collect(k, i):
        res, codes = ring.poll_txns(k, len(batches[i][1]), want_codes=True)
        same(res, exps[i][0])
        assert np.array_equal(codes, exps[i][1])

    collect(tk[1], 1)                      # the second first
    k3 = ring.submit_txns(b3, t3)          # into the slot it freed
    assert k3 > tk[2]
    collect(tk[2], 2)
    collect(k3, 3)
    collect(tk[0], 0)


def test_descriptor_and_transaction_batches_interleaved(ring, ref, txns12):
    """one ring, one ticket counter, two kinds of batch: each collected by its own poll;
    the cross polls are ERR_ARG and leave the ticket valid; a drain takes either"""
    L = fa.lib()
    blob, t = mixed(txns12, 100, 200, [9, 50])
    exp, ecodes = ring_expect(ref, blob, t)
    eres, ecd, edesc, _ = expect(ref, blob, t)
    k_d = ring.submit(blob, edesc)
    k_t = ring.submit_txns(blob, t)
    k_d2 = ring.submit(blob, edesc[:17])
    assert k_d < k_t < k_d2
    out = np.full(len(edesc), 77, np.int32)
    res = np.zeros(len(t), fa.TXN_RESULT_DTYPE)
    for block in (0, 1):
        assert L.fd_ed25519_gpu_poll(ring._h, k_t, P(out), block) == fa.ERR_ARG
        assert L.fd_ed25519_gpu_poll_txns(ring._h, k_d, P(res), None, block) == fa.ERR_ARG
    assert (out == 77).all() and not res.view(np.uint8).any()
    got, codes = ring.poll_txns(k_t, len(t), want_codes=True)
    same(got, exp)
    assert np.array_equal(codes, ecodes)
    assert ring.poll(k_d, out) and np.array_equal(out, ecd)
    out2 = np.zeros(17, np.int32)
    assert ring.poll(k_d2, out2) and np.array_equal(out2, ecd[:17])
    # fd_ed25519_gpu_poll( ticket, NULL ) drains a transaction ticket
    k = ring.submit_txns(blob, t)
    assert L.fd_ed25519_gpu_poll(ring._h, k, None, 1) == 1
    assert L.fd_ed25519_gpu_poll_txns(ring._h, k, P(res), None, 1) == fa.ERR_ARG
    del ring._pending_txns[k]
    tickets = [ring.submit_txns(blob, t) for _ in range(3)]           # all three slots are back
    for k in tickets:
        same(ring.poll_txns(k, len(t)), exp)


# ---------------------------------------------------------------- 4. where the bytes lie

def slot_states(eng):
    st = (ctypes.c_int * 8)()
    f = fa.lib().fd_ed25519_gpu_slot_states
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    f.restype = ctypes.c_int
    n = f(eng._h, st, 8)
    return list(st)[:n]


def test_where_the_bytes_lie(ring, ref, txns12):
    """an ordinary array, a registered region (read in place) and a slot's staged buffer
    (no copy) give the same results; a slot kept by the poll is not handed out until it
    is unstaged"""
    L = fa.lib()
    blob, t = mixed(txns12, 200, 330, [3, 64, 129])
    exp, ecodes = ring_expect(ref, blob, t)
    plain = ring_run(ring, blob, t)
    region = np.zeros(1 << 20, np.uint8)
    region[4096:4096 + len(blob)] = blob
    ring.register(region)
    try:
        inplace = ring_run(ring, region[4096:4096 + len(blob)], t)
    finally:
        ring.unregister(region)
    hb, hd = ctypes.c_void_p(0), ctypes.c_void_p(0)
    assert L.fd_ed25519_gpu_stage(ring._h, ctypes.byref(hb), ctypes.byref(hd)) == 0
    ctypes.memmove(hb.value, blob.ctypes.data, blob.nbytes)
    ticket = ctypes.c_ulong(0)
    assert L.fd_ed25519_gpu_submit_txns(ring._h, len(t), hb, blob.nbytes, P(t), ctypes.byref(ticket)) == 0
    res = np.zeros(len(t), fa.TXN_RESULT_DTYPE)
    codes = np.zeros(len(ecodes), np.int32)
    assert L.fd_ed25519_gpu_poll_txns(ring._h, ticket.value, P(res), P(codes), 1 | POLL_KEEP) == 1
    for got in (plain, inplace, (res, codes)):
        same(got[0], exp)
        assert np.array_equal(got[1], ecodes)
    # the kept slot: no ticket, staged; its bytes are still the caller's
    assert sorted(s & 3 for s in slot_states(ring)) == [0, 0, 2]
    assert bytes((ctypes.c_ubyte * 64).from_address(hb.value)) == blob[:64].tobytes()
    tk = [ring.try_submit_txns(blob, t) for _ in range(3)]
    assert tk[0] is not None and tk[1] is not None and tk[2] is None
    L.fd_ed25519_gpu_unstage(ring._h, hb)
    tk[2] = ring.try_submit_txns(blob, t)
    assert tk[2] is not None
    for k in tk:
        same(ring.poll_txns(k, len(t)), exp)
    assert all(s & 3 == 0 for s in slot_states(ring))


# ---------------------------------------------------------------- 5. schedules and modes

def adversarial(txns12, lo, target, n_small, n_noncanon):
    """about `target` signatures: a Q1 early-accept S, small-order and non-canonical
    signers, two bad signatures in one transaction, an unparsed claim, the rest valid"""
    five = [p for p in txns12[lo:] if 5 <= p[0] <= 8]
    rest = [p for p in txns12[lo:] if p[0] < 5]
    q1 = bytearray(five[0])
    q1[1 + 64 * 3 + 63] = 0x10                     # S >= L that the reference's AVX build accepts as a scalar
    ps = [bytes(q1), corrupt(five[1], a=4, b=2), unparsed_claim(rest[0])]
    encs = corpus.small_order_encodings()[:n_small]
    encs += [b"\xff" * 31 + b"\x7f", b"\xee" + b"\xff" * 30 + b"\x7f", b"\xed" + b"\xff" * 30 + b"\xff"][:n_noncanon]
    for src, enc in zip(five[2:], encs):
        p = bytearray(src)
        ao = txn.parse(bytes(p))["acct_addr_off"]
        p[ao + 32 * 4:ao + 32 * 5] = enc           # signer 4
        ps.append(bytes(p))
    s = sum(p[0] for p in ps)
    for p in rest[1:]:
        if s >= target:
            break
        ps.insert(len(ps) // 2, p)
        s += p[0]
    return txn.pack(ps, gap=2, first=5)


@pytest.fixture(scope="module")
def sched_batches(txns12):
    return [adversarial(txns12, 0, 56, 2, 1), adversarial(txns12, 100, 600, 6, 3)]


def test_schedules_and_modes(ring, ref, refp, oracle, sched_batches):
    """the oct, quad and uniform schedules (dsm_oct_max, dsm_quad_max set to 0 in turn), in
    the AVX, portable and strict modes, on ~60 and ~600 signatures"""
    modes = [(fa.MODE_AVX, None), (fa.MODE_PORTABLE, lambda b: ref_codes(refp, "refp_verify_batch", b)),
             (fa.MODE_STRICT, lambda b: ref_codes(oracle, "oracle_verify_batch_strict", b))]
    exps = {m: [ring_expect(ref, blob, t, fn) for blob, t in sched_batches] for m, fn in modes}
    n60, n600 = (len(e[1]) for e in exps[fa.MODE_AVX])
    assert 40 <= n60 <= 64 and 500 <= n600 <= 700
    assert not np.array_equal(exps[fa.MODE_AVX][1][1], exps[fa.MODE_PORTABLE][1][1])     # the builds do differ here
    assert not np.array_equal(exps[fa.MODE_AVX][1][1], exps[fa.MODE_STRICT][1][1])
    oct0, quad0 = ring.dsm_oct_max, ring.dsm_quad_max
    assert n60 <= oct0 < n600 <= quad0
    try:
        for oct_max, quad_max in ((oct0, quad0), (0, quad0), (0, 0)):
            ring.dsm_oct_max, ring.dsm_quad_max = oct_max, quad_max
            for m, _ in modes:
                ring.mode = m
                for (blob, t), (exp, ecodes) in zip(sched_batches, exps[m]):
                    got, codes = ring_run(ring, blob, t)
                    same(got, exp)
                    assert np.array_equal(codes, ecodes), (oct_max, quad_max, m)
    finally:
        ring.mode = fa.MODE_AVX
        ring.dsm_oct_max, ring.dsm_quad_max = oct0, quad0


# ---------------------------------------------------------------- 6. reserve

def test_reserve_allocates_the_slots_scratch(ref, txns12):
    """after txns_reserve a submit allocates nothing (the engine counts the slots whose
    scratch it allocated); without one the first submit does"""
    blob, t = txn.pack(txns12[:9], gap=1, first=1)
    exp, ecodes = ring_expect(ref, blob, t)
    for reserve in (True, False):
        e = fa.Engine(0, 512, 1 << 16, depth=4)
        try:
            assert e.txn_ring_allocs() == 0
            if reserve:
                e.txns_reserve(64)
                assert e.txn_ring_allocs() == 4
            for _ in range(2):
                tickets = [e.submit_txns(blob, t) for _ in range(4)]
                assert e.txn_ring_allocs() == 4
                for k in tickets:
                    got, codes = e.poll_txns(k, len(t), want_codes=True)
                    same(got, exp)
                    assert np.array_equal(codes, ecodes)
            e.txns_reserve(128)
            assert e.txn_ring_allocs() == 4
        finally:
            e.close()


def test_large_batch_codes_by_copy(ref, txns12):
    """past out_direct_max (4,096) the codes come back by a D2H copy behind the reduce"""
    e = fa.Engine(0, 6000, 1 << 20, depth=2)
    try:
        ps = exactly(txns12, 4500)
        ps[10] = corrupt(ps[10], b=0)
        ps[len(ps) - 1] = unparsed_claim(ps[len(ps) - 1])
        blob, t = txn.pack(ps, gap=0, first=0)
        got, codes = check(e, ref, blob, t, packed=False)
        assert len(codes) == 4500 and got["status"][10] != 0 and got["status"][-1] == fa.ERR_TXN
    finally:
        e.close()
