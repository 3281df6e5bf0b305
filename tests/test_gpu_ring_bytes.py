"""The engine ring's descriptor path at the C ABI (fd_ed25519_gpu_try_submit2 /
_try_submit / _stage / _poll, fd_ed25519_gpu_host.cpp): where a batch's bytes
may lie, and the ring rules both kinds of ticket share.

One engine (4,096 signatures, 1 MiB, depth 3) and one corpus.adversarial batch
of 4,096 with invalid signatures mixed in; n = 40 and n = 200 are its first
signatures.  40 is at most early_max = 64 (the eight-lane DSM, codes taken as
they land); 200 is past it (the quad-lane DSM, the completion event): the
smallest sizes on either side of the only size-dependent branches of the
placement code.  Expected codes come from conftest.oracle_batch( ref ) alone,
transaction results from the reference through test_gpu_txn_ring.ring_expect;
every comparison is exact.

Before each placement every slot's device buffer is overwritten by a batch of
other bytes, so a copy that is left out cannot be made up for by what the
slot's last batch left there.  Slot states are read through
fd_ed25519_gpu_slot_states: bit value 1 a ticket, 2 staged, 4 retiring."""
import ctypes
import time

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P, oracle_batch
from firedancer_amd import corpus, txn
from test_gpu_txn import same
from test_gpu_txn_ring import ring_expect, slot_states

pytestmark = pytest.mark.gpu

MAX_SIGS, MAX_BLOB, DEPTH = 4096, 1 << 20, 3
POLL_KEEP = 2                      # FD_ED25519_GPU_POLL_KEEP
MSG = 128
STRIDE = 96 + MSG                  # corpus.simple: R||S (64) | key (32) | message
SIZES = [40, 200]
DSZ = fa.DESC_DTYPE.itemsize
MTU = corpus.TXN_MTU


@pytest.fixture(scope="module")
def eng():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    e = fa.Engine(0, MAX_SIGS, MAX_BLOB, depth=DEPTH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(ref):
    """(the batch of 4,096, the reference's codes): valid and invalid among the first 40"""
    b = corpus.adversarial(MAX_SIGS, MSG, seed=61, invalid_frac=0.25)
    exp = oracle_batch(ref, b)
    exp.setflags(write=False)
    assert exp[:40].any() and (exp[:40] == 0).any() and exp[40:200].any()
    assert len(b.blob) <= MAX_BLOB
    return b, exp


@pytest.fixture(scope="module")
def txns(ref):
    """2,048 transactions claiming 4,096 signatures (entries share 512 two-signature
    payloads, as many as keep the blob inside the engine's) -> (blob, entries, results, codes)"""
    b = corpus.solana_txns(1024, seed=62, p2=1.0)
    ps = [bytes(b.blob[i * MTU:(i + 1) * MTU]) for i in range(512)]
    blob, t = txn.pack(ps, gap=1, first=1)
    t = t[np.arange(2048) % len(t)].copy()
    res, codes = ring_expect(ref, blob, t)
    assert len(codes) == 4096 and not res["status"].any() and len(blob) <= MAX_BLOB
    return blob, t, res, codes


def head(batch, n):
    """the first n signatures: (blob bytes, descriptors, expected codes)"""
    b, exp = batch
    return b.blob[:n * STRIDE], b.desc[:n], exp[:n]


# ---------------------------------------------------------------- the C ABI

def addr(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def submit2(eng, n, blob, sz, blob2, sz2, desc):
    """fd_ed25519_gpu_try_submit2 on raw addresses -> (return value, ticket)"""
    k = ctypes.c_ulong(0)
    r = fa.lib().fd_ed25519_gpu_try_submit2(eng._h, n, blob, sz, blob2, sz2, desc, ctypes.byref(k))
    return r, k.value


def poll(eng, ticket, n, block=1):
    out = np.full(max(n, 1), 99, np.int32)
    r = fa.lib().fd_ed25519_gpu_poll(eng._h, ticket, P(out), block)
    return r, out[:n]


def poll_txns(eng, ticket, n_txn, n_sig, block=1):
    res, codes = np.zeros(n_txn, fa.TXN_RESULT_DTYPE), np.full(n_sig, 99, np.int32)
    r = fa.lib().fd_ed25519_gpu_poll_txns(eng._h, ticket, P(res), P(codes), block)
    return r, res, codes


def stage(eng):
    hb, hd = ctypes.c_void_p(0), ctypes.c_void_p(0)
    r = fa.lib().fd_ed25519_gpu_stage(eng._h, ctypes.byref(hb), ctypes.byref(hd))
    return r, hb, hd


def unstage(eng, hb):
    fa.lib().fd_ed25519_gpu_unstage(eng._h, hb)


def all_free(eng):
    """every slot without ticket and stage.  A slot whose codes were taken early keeps its
    ticket until its event has completed (microseconds) and a caller that looks for a slot
    reclaims it: a stage that is handed straight back is such a caller"""
    t0 = time.monotonic()
    while True:
        r, hb, _ = stage(eng)
        if r == 0:
            unstage(eng, hb)
        st = slot_states(eng)
        if len(st) == DEPTH and all(s & 3 == 0 for s in st):
            return True
        if time.monotonic() - t0 > 2.0:
            return False


def desc_bufs(eng):
    """the three slots' pinned descriptor buffers (what fd_ed25519_gpu_stage lends), as arrays"""
    got = [stage(eng) for _ in range(DEPTH)]
    assert all(r == 0 for r, _, _ in got)
    for _, hb, _ in got:
        unstage(eng, hb)
    return [np.ctypeslib.as_array((ctypes.c_uint8 * (MAX_SIGS * DSZ)).from_address(hd.value)) for _, _, hd in got]


def scrub(eng, n):
    """other bytes into every slot's device blob and 0xEE over every pinned descriptor buffer"""
    junk = np.full(n * STRIDE, 0xA5, np.uint8)
    d = np.zeros(n, fa.DESC_DTYPE)
    d["pub_off"], d["msg_off"], d["msg_sz"] = 64, 96, 32
    ks = [submit2(eng, n, P(junk), junk.nbytes, None, 0, P(d)) for _ in range(DEPTH)]
    assert all(r == 1 for r, _ in ks), ks
    for _, k in ks:
        assert fa.lib().fd_ed25519_gpu_poll(eng._h, k, None, 1) == 1
    assert all_free(eng), slot_states(eng)
    bufs = desc_bufs(eng)
    for b in bufs:
        b[:n * DSZ] = 0xEE
    return bufs


def run(eng, n, blob, sz, blob2, sz2, desc, exp):
    r, k = submit2(eng, n, blob, sz, blob2, sz2, desc)
    assert r == 1, (r, fa.last_error())
    r, out = poll(eng, k, n)
    assert r == 1, (r, fa.last_error())
    bad = np.nonzero(out != exp)[0]
    assert len(bad) == 0, f"{len(bad)} codes differ, the first at {bad[:8].tolist()}"
    assert all_free(eng), slot_states(eng)


def written(bufs, n):
    """how many of the pinned descriptor buffers no longer hold scrub's 0xEE"""
    return sum(bool((b[:n * DSZ] != 0xEE).any()) for b in bufs)


def splits(n):
    """byte 1, the middle of a signature, the middle of a message, the last byte"""
    return [1, 3 * STRIDE + 30, 5 * STRIDE + 96 + 50, n * STRIDE - 1]


# ---------------------------------------------------------------- 1. where the bytes lie

@pytest.mark.parametrize("n", SIZES)
def test_ordinary_arrays_and_the_staged_buffers(eng, batch, n):
    """placements 1 and 2: both are one copy from the slot's pinned blob; the descriptors
    travel behind the blob, not through the mapped descriptor buffer"""
    blob, desc, exp = head(batch, n)
    bufs = scrub(eng, n)
    run(eng, n, P(blob), blob.nbytes, None, 0, P(desc), exp)
    assert written(bufs, n) == 0
    r, hb, hd = stage(eng)
    assert r == 0
    ctypes.memmove(hb.value, blob.ctypes.data, blob.nbytes)
    ctypes.memmove(hd.value, desc.ctypes.data, desc.nbytes)
    run(eng, n, hb, blob.nbytes, None, 0, hd, exp)          # the submit consumes the stage
    assert written(bufs, n) == 1                            # by this test, above


@pytest.mark.parametrize("n", SIZES)
def test_a_registered_blob(eng, batch, n):
    """placements 3, 4 and 5: the blob is read where it lies.  Descriptors in an ordinary
    array, or in the region but not at the packed offset, go through one slot's mapped
    descriptor buffer; at fd_ed25519_gpu_desc_offset( blob_sz ) behind the blob and its
    zero pad the batch is one copy and no descriptor buffer is written"""
    L = fa.lib()
    L.fd_ed25519_gpu_desc_offset.argtypes, L.fd_ed25519_gpu_desc_offset.restype = [ctypes.c_ulong], ctypes.c_ulong
    blob, desc, exp = head(batch, n)
    sz = blob.nbytes
    doff = L.fd_ed25519_gpu_desc_offset(sz)
    assert doff >= sz + 64 and doff % 16 == 0
    region = np.zeros(1 << 19, np.uint8)
    at, apart = 4096, 1 << 18
    region[at:at + sz] = blob
    region[apart:apart + desc.nbytes] = desc.view(np.uint8)
    region[at + doff:at + doff + desc.nbytes] = desc.view(np.uint8)
    eng.register(region)
    try:
        for d, mapped in ((P(desc), 1), (addr(region, apart), 1), (addr(region, at + doff), 0)):
            bufs = scrub(eng, n)
            run(eng, n, addr(region, at), sz, None, 0, d, exp)
            assert written(bufs, n) == mapped
            if mapped:
                hit = [b for b in bufs if (b[:n * DSZ] != 0xEE).any()][0]
                assert hit[:n * DSZ].tobytes() == desc.tobytes()
    finally:
        eng.unregister(region)


@pytest.mark.parametrize("where", ["registered", "ordinary", "first_registered"])
@pytest.mark.parametrize("n", SIZES)
def test_two_pieces(eng, batch, n, where):
    """placements 6, 7 and 8: the batch's bytes are piece 1 then piece 2, the second lying
    before the first as a ring wrap leaves them; both registered (two copies from where
    they lie), neither, or only the first (staged)"""
    blob, desc, exp = head(batch, n)
    sz = blob.nbytes
    region = np.zeros(1 << 19, np.uint8)
    other = np.zeros(1 << 19, np.uint8)
    if where != "ordinary":
        eng.register(region)
    try:
        for cut in splits(n):
            assert 0 < cut < sz
            first, second = (1 << 18) + 32, 64
            region[first:first + cut] = blob[:cut]
            two = other if where == "first_registered" else region
            two[second:second + sz - cut] = blob[cut:]
            bufs = scrub(eng, n)
            run(eng, n, addr(region, first), cut, addr(two, second), sz - cut, P(desc), exp)
            assert written(bufs, n) == (1 if where == "registered" else 0)
            region[:] = 0
            other[:] = 0
    finally:
        if where != "ordinary":
            eng.unregister(region)


def test_the_edges_of_the_argument_check(eng, batch):
    """placement 9.  An empty batch (blob_sz 0, n 0) is taken: a ticket, and a poll that
    returns 1 and writes no code.  A second piece past what is left of max_blob is refused
    with ERR_ARG before a slot is looked at"""
    r, k = submit2(eng, 0, None, 0, None, 0, None)
    assert r == 1 and k
    r, out = poll(eng, k, 1)
    assert r == 1 and out[0] == 99
    assert all_free(eng), slot_states(eng)
    blob, desc, _ = head(batch, 40)
    r, k = submit2(eng, 40, P(blob), blob.nbytes, P(blob), MAX_BLOB - blob.nbytes + 1, P(desc))
    assert (r, k) == (fa.ERR_ARG, 0)
    assert all(s & 3 == 0 for s in slot_states(eng))


# ---------------------------------------------------------------- 2. ring rules

@pytest.mark.parametrize("n", SIZES)
def test_poll_keep_lends_the_slot_back(eng, batch, n):
    """a staged batch polled with POLL_KEEP: the slot stays the caller's (staged; at 40,
    where the codes are taken early, it may still be retiring), its bytes untouched, and
    it is not handed out until it is unstaged"""
    L = fa.lib()
    blob, desc, exp = head(batch, n)
    assert all_free(eng)
    r, hb, hd = stage(eng)
    assert r == 0
    ctypes.memmove(hb.value, blob.ctypes.data, blob.nbytes)
    ctypes.memmove(hd.value, desc.ctypes.data, desc.nbytes)
    k = ctypes.c_ulong(0)
    assert L.fd_ed25519_gpu_try_submit(eng._h, n, hb, blob.nbytes, hd, ctypes.byref(k)) == 1
    r, out = poll(eng, k.value, n, 1 | POLL_KEEP)
    assert r == 1 and np.array_equal(out, exp)
    st = slot_states(eng)
    assert sorted(s & 2 for s in st) == [0, 0, 2], st
    for s in st:
        if s & 2:
            assert (s & 1) == 0 or (s & 4), st              # a ticket only while it retires
        else:
            assert s & 3 == 0, st
    assert bytes((ctypes.c_ubyte * 64).from_address(hb.value)) == blob[:64].tobytes()
    ks = [submit2(eng, n, P(blob), blob.nbytes, None, 0, P(desc)) for _ in range(3)]
    assert [r for r, _ in ks] == [1, 1, 0], ks
    unstage(eng, hb)
    ks[2] = submit2(eng, n, P(blob), blob.nbytes, None, 0, P(desc))
    assert ks[2][0] == 1
    for _, t in ks:
        r, out = poll(eng, t, n)
        assert r == 1 and np.array_equal(out, exp)
    assert all_free(eng), slot_states(eng)


def _timed_out_then_collected(eng, submit, collect):
    """a 1 us host wait bound (nothing is provoked on the device): the blocking poll gives
    up with ERR_GPU, the ticket stays valid, and with the bound restored the same ticket
    gives its results"""
    old = eng.timeout_ns
    eng.timeout_ns = 1000
    try:
        k = submit()
        r = collect(k)[0]
    finally:
        eng.timeout_ns = old
    assert r != 1, "the 1 us timeout never fired: the test exercised nothing"
    assert r == fa.ERR_GPU, (r, fa.last_error())
    assert sum(s & 1 for s in slot_states(eng)) == 1
    got = collect(k)
    assert got[0] == 1, (got[0], fa.last_error())
    assert all_free(eng), slot_states(eng)
    return got


@pytest.mark.parametrize("n", [40, 4096])
def test_a_timed_out_poll_leaves_a_descriptor_ticket_valid(eng, batch, n):
    """at 4,096 the wait for the completion event times out, at 40 the wait for the codes"""
    blob, desc, exp = head(batch, n)
    assert all_free(eng)

    def submit():
        r, k = submit2(eng, n, P(blob), blob.nbytes, None, 0, P(desc))
        assert r == 1
        return k
    _, out = _timed_out_then_collected(eng, submit, lambda k: poll(eng, k, n))
    assert np.array_equal(out, exp)


def test_a_timed_out_poll_leaves_a_transaction_ticket_valid(eng, txns):
    blob, t, eres, ecodes = txns
    assert all_free(eng)
    _, res, codes = _timed_out_then_collected(eng, lambda: eng.submit_txns(blob, t), lambda k: poll_txns(eng, k, len(t), len(ecodes)))
    eng._pending_txns.clear()
    same(res, eres)
    assert np.array_equal(codes, ecodes)


def test_a_poll_before_completion_returns_0(eng, batch, txns):
    """both kinds at 4,096 signatures (about 0.8 ms on the device): the non-blocking poll
    that follows the submit finds the batch in flight and returns 0; each ticket is refused
    by the other kind's poll and stays valid; a blocking poll then gives the results"""
    L = fa.lib()
    blob, desc, exp = head(batch, MAX_SIGS)
    tb, t, eres, ecodes = txns
    assert all_free(eng)
    r, kd = submit2(eng, MAX_SIGS, P(blob), blob.nbytes, None, 0, P(desc))
    assert r == 1
    r0, out0 = poll(eng, kd, MAX_SIGS, 0)
    kt = eng.submit_txns(tb, t)
    r1 = poll_txns(eng, kt, len(t), len(ecodes), 0)[0]
    assert (r0, r1) == (0, 0) and (out0 == 99).all()
    for block in (0, 1):
        r, out = poll(eng, kt, MAX_SIGS, block)             # a transaction ticket, codes wanted
        assert r == fa.ERR_ARG and (out == 99).all()
        r, res, codes = poll_txns(eng, kd, len(t), len(ecodes), block)
        assert r == fa.ERR_ARG and not res.view(np.uint8).any() and (codes == 99).all()
    r, out = poll(eng, kd, MAX_SIGS)
    assert r == 1 and np.array_equal(out, exp)
    r, res, codes = poll_txns(eng, kt, len(t), len(ecodes))
    eng._pending_txns.clear()
    assert r == 1
    same(res, eres)
    assert np.array_equal(codes, ecodes)
    assert L.fd_ed25519_gpu_poll(eng._h, kd, None, 1) == fa.ERR_ARG   # collected: the tickets are gone
    assert all_free(eng), slot_states(eng)
