"""What carries message bytes into SHA-512, on the device, byte for byte.

The grid of tests/hash_grid.py (every message length 0..401 at every start
alignment mod 16, giants up to 65,537 bytes, dead rows, in a ragged and a
sorted order; tests/test_hash_grid.py holds the conditions on it) through
  a  fd_k_prep (fd_sha_stage, fd_sha_words, PRE = 64): k = SHA-512(R||A||M) mod L
     of every pending row against hashlib, the dead rows' statuses
  b  fd_k_front's wave pair (fd_sha_fetch, the wave-uniform nblk_max against
     each lane's own nblk, dead lanes): op rows equal those of the same launch
     fed hashlib's digests
  c  verify_packed on five schedules: the reference's code on every row, the
     flip rows (one message bit at a block, chunk or tail edge) included
  d  the ring in four batches, and verify_dev on a tensor of exactly
     blob_sz + 16 bytes whose pad is 0x00 and then 0xA5
  e  fd_k_sha512_batch (PRE = 0) through fd_ed25519_gpu_sha512_packed with the
     test's own descriptors, SHA-512 and SHA-384 against hashlib
  f  sign_packed at the grid's message offsets against the host signer
Every comparison is exact bytes or exact codes on every row; none is left out.
Rows h1 and h2 of the DESIGN test table."""
import hashlib

import numpy as np
import pytest

import firedancer_amd as fa
import hash_grid as hg
from test_gpu_chosen_scalars import set_schedule

pytestmark = pytest.mark.gpu

L = hg.L
SCHEDULES = ("uniform", "pooled", "quad", "oct", "default")


@pytest.fixture(scope="module")
def g(ref):
    g = hg.grid(ref)
    for p in (g.ragged, g.sorted):
        if not hasattr(p, "dig"):
            p.dig = hg.digests(p)
    return g


@pytest.fixture(scope="module")
def eng():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    e = fa.Engine(0, 8192, 1 << 23)
    yield e
    e.close()


@pytest.fixture
def sched(eng):
    yield lambda name: set_schedule(eng, name)
    set_schedule(eng, "default")


def describe(p, j):
    """the offending row, for an assertion message"""
    return (f"row {int(j)} kind {int(p.kind[j])} sz {int(p.desc['msg_sz'][j])} at {int(p.desc['msg_off'][j]) % 16} mod 16, "
            f"{int(hg.nblk(p.sz[j]))} blocks, wave {int(j) // 64}",)


def check_codes(p, got, what):
    bad = np.nonzero(got != p.exp)[0]
    assert len(bad) == 0, (what, len(bad), [describe(p, j) + (int(p.exp[j]), int(got[j])) for j in bad[:6]])
    assert len(got) == len(p)


# ------------------------------------------------------------------ a
@pytest.mark.parametrize("order", ["ragged", "sorted"])
def test_prep_k_is_hashlib_mod_L(eng, sched, g, order):
    p = getattr(g, order)
    sched("uniform")
    k, st = eng.debug_k(p.blob, p.desc)
    pend = p.kind <= hg.GIANT
    want_st = np.where(pend, 1, p.exp)              # a dead row's status is its code
    bad = np.nonzero(st != want_st)[0]
    assert len(bad) == 0, [describe(p, j) + (int(want_st[j]), int(st[j])) for j in bad[:6]]
    want = np.zeros((len(p), 32), np.uint8)
    for j in np.nonzero(pend)[0]:
        want[j] = np.frombuffer((int.from_bytes(p.dig[j].tobytes(), "little") % L).to_bytes(32, "little"), np.uint8)
    bad = np.nonzero((k != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [describe(p, j) for j in bad[:6]])
    assert pend.sum() == 6456


# ------------------------------------------------------------------ b
def stages_equal(eng, p, rows, what):
    desc = p.desc[rows]
    s1 = eng.debug_stages(p.blob, desc, None)
    s2 = eng.debug_stages(p.blob, desc, p.dig[rows])
    assert s1.schedule == s2.schedule == what[0]
    pend = p.kind[rows] <= hg.GIANT
    bad = np.nonzero(s1.status != s2.status)[0]
    assert len(bad) == 0, (what, "status", [describe(p, rows[j]) for j in bad[:6]])
    assert (s1.status == np.where(pend, 1, p.exp[rows])).all()
    bad = np.nonzero(pend & ((s1.op_start != s2.op_start) | (s1.ops != s2.ops).any(axis=1)))[0]
    assert len(bad) == 0, (what, "op rows", len(bad), [describe(p, rows[j]) for j in bad[:6]])
    assert (s1.codes == p.exp[rows]).all() and (s2.codes == p.exp[rows]).all()


@pytest.mark.parametrize("order", ["ragged", "sorted"])
def test_front_wave_pair_is_hashlib(eng, sched, g, order):
    sched("quad")
    p = getattr(g, order)
    stages_equal(eng, p, np.arange(len(p)), ("quad", order))


@pytest.mark.parametrize("n", [1, 5, 32, 33, 64])
def test_front_small_batches(eng, sched, g, n):
    """n <= 32: S recoded ahead by an idle wave; n <= 64: the oct schedule.  Each slice
    holds a giant, a zero-length row and a dead row of every kind (n = 1: a giant
    alone, then a zero-length row alone), the rest taken from the ragged order"""
    p = g.ragged
    giant = np.nonzero(p.kind == hg.GIANT)[0]
    zero = np.nonzero((p.kind == hg.GRID) & (p.sz == 0))[0]
    for rep in range(3):
        if n == 1:
            picks = [[giant[rep]], [zero[rep]], [giant[-1 - rep]]][rep]
        else:
            head = [giant[rep], zero[rep]] + [np.nonzero(p.kind == d)[0][rep] for d in (hg.DEAD_SIG, hg.DEAD_Q1, hg.DEAD_PAST, hg.DEAD_WRAP)]
            picks = (head + [j for j in range(200 * rep, 200 * rep + 64) if j not in head])[:n]
            picks = list(np.roll(picks, 7 * rep))           # the giant on another lane each time
        rows = np.array(picks)
        assert len(set(picks)) == n
        for name in ("quad", "oct"):
            sched(name)
            stages_equal(eng, p, rows, (name, n, rep))


# ------------------------------------------------------------------ c
@pytest.mark.parametrize("name", ["ragged", "sorted", "flips"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_codes(eng, sched, g, schedule, name):
    sched(schedule)
    p = getattr(g, name)
    check_codes(p, eng.verify_packed(p.blob, p.desc), (schedule, name))


# ------------------------------------------------------------------ d
def test_ring_four_batches(eng, g):
    p = g.ragged
    cuts = np.linspace(0, len(p), 5).astype(int)
    got = np.full(len(p), 99, np.int32)
    for a in (0, 2):                                # two in flight
        tickets = [(eng.submit(p.blob, p.desc[cuts[i]:cuts[i + 1]]), i) for i in (a, a + 1)]
        for t, i in tickets:
            out = np.full(cuts[i + 1] - cuts[i], 99, np.int32)
            assert eng.poll(t, out)
            got[cuts[i]:cuts[i + 1]] = out
    check_codes(p, got, "ring")


@pytest.mark.parametrize("schedule", ["uniform", "quad"])
def test_device_resident_pad_is_not_hashed(eng, sched, g, schedule):
    """verify_dev reads the caller's memory: blob_sz bytes and the 16 pad bytes the
    header asks for, nothing zeroed by the engine.  The last live message ends at
    blob_sz, so its last fetch chunk reaches into the pad"""
    import torch
    p = g.ragged
    sched(schedule)
    n, bsz = len(p), p.blob.nbytes
    desc = torch.from_numpy(p.desc.view(np.uint8).copy()).cuda()
    runs = []
    for fill in (0x00, 0xA5):
        blob = torch.from_numpy(np.concatenate([p.blob, np.full(16, fill, np.uint8)])).cuda()
        assert blob.numel() == bsz + 16
        out = torch.full((n,), 99, dtype=torch.int32, device="cuda")
        eng.verify_dev(n, blob.data_ptr(), bsz, desc.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
        check_codes(p, runs[-1], (schedule, "verify_dev, pad", hex(fill)))
    assert (runs[0] == runs[1]).all()


# ------------------------------------------------------------------ e
@pytest.fixture(scope="module")
def plain(g):
    """every length 0..401 at every alignment, and the giants' lengths, as plain
    messages in the ragged order's blob: its message descriptors, nothing padded"""
    p = g.ragged
    rows = np.nonzero(p.kind <= hg.GIANT)[0]
    desc = np.zeros(len(rows), fa.DESC_DTYPE)
    desc["msg_off"], desc["msg_sz"] = p.desc["msg_off"][rows], p.desc["msg_sz"][rows]
    msgs = [p.blob[int(o):int(o) + int(s)].tobytes() for o, s in zip(desc["msg_off"], desc["msg_sz"])]
    pairs = set(zip((desc["msg_sz"] % 128).tolist(), (desc["msg_off"] % 16).tolist()))
    assert len(pairs) == 128 * 16 and len(rows) == 6456
    assert (desc["msg_off"].astype(np.int64) + desc["msg_sz"]).max() == p.blob.nbytes
    return p, rows, desc, msgs


@pytest.mark.parametrize("is384", [False, True])
def test_plain_sha512_any_offset(eng, plain, is384):
    p, rows, desc, msgs = plain
    hsz = 48 if is384 else 64
    out = np.zeros((len(desc), hsz), np.uint8)
    err = fa.lib().fd_ed25519_gpu_sha512_packed(eng._h, len(desc), fa._p(p.blob), p.blob.nbytes, fa._p(desc), fa._p(out), int(is384))
    assert err == 0, fa.last_error()
    h = hashlib.sha384 if is384 else hashlib.sha512
    want = np.frombuffer(b"".join(h(m).digest() for m in msgs), np.uint8).reshape(len(msgs), hsz)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [describe(p, rows[j]) for j in bad[:6]])


# ------------------------------------------------------------------ f
def test_sign_at_grid_offsets(eng, g):
    """one sign_packed call over the live rows: seeds appended after the blob at a
    33-byte stride, the public key derived on the device (even rows) or read from the
    row's pub_off (odd rows): the host signer's 64 bytes on every row"""
    p = g.ragged
    rows = np.nonzero(p.kind <= hg.GIANT)[0]
    n = len(rows)
    assert n <= 8192
    bsz = p.blob.nbytes
    blob = np.concatenate([p.blob, np.random.default_rng(5).integers(0, 256, 33 * n + 1, dtype=np.uint8)])
    so = bsz + 1 + 33 * np.arange(n)
    blob[so[:, None] + np.arange(32)[None, :]] = g.rows.seed[p.row[rows]]
    sd = np.zeros(n, fa.SIGN_DESC_DTYPE)
    sd["seed_off"], sd["msg_off"], sd["msg_sz"] = so, p.desc["msg_off"][rows], p.desc["msg_sz"][rows]
    sd["pub_off"] = np.where(np.arange(n) % 2 == 0, fa.SIGN_DERIVE, p.desc["pub_off"][rows])
    sig, pub, codes = eng.sign_packed(blob, sd)
    assert (codes == 0).all()
    bad = np.nonzero((sig != p.sig[rows]).any(axis=1) | (pub != p.pub[rows]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [describe(p, rows[j]) for j in bad[:6]])
