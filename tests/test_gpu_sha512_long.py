"""SHA-512 / SHA-384 of messages of any size on the device
(include/fd_sha512_gpu.h): fd_sha512_gpu_batch_fini and
fd_ed25519_gpu_sha512_ptrs stream a message no staged chunk can hold through
the engine's blob in pieces (fd_k_sha512_pieces, one lane per message).

The engines here are small, so that "long" means a few kilobytes and every
case takes well under a second; the group size G and the blocks per launch C
come from the library's own geometry (fd_sha512_gpu_long_geometry), not from
formulas restated here.  Digests are compared for equality with hashlib,
and with the reference's fd_sha512 / fd_sha384 (oracle/_ref) on top."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

import firedancer_amd as fa

pytestmark = pytest.mark.gpu

BLOB = 2048
FILL = b"\xaa" * 64


def expect(msg, is384):
    return (hashlib.sha384 if is384 else hashlib.sha512)(msg).digest()


def ref_hash(ref, msg, is384):
    fn = ref.ref_sha384 if is384 else ref.ref_sha512
    fn.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_void_p]
    out = ctypes.create_string_buffer(64)
    fn(msg, len(msg), out)
    return out.raw[:48 if is384 else 64]


def rand_msgs(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in sizes]


class Batch:
    """one fd_sha512_gpu_batch_t; run() queues, finishes and returns every
    64-byte out buffer (pre-filled with 0xAA) whole"""

    def __init__(self, eng, is384):
        self.L = fa.lib()
        self.is384 = is384
        self.b = self.L.fd_sha512_gpu_batch_new(eng._h, 1 if is384 else 0)
        assert self.b

    def queue(self, msgs):
        L = self.L
        bufs = [ctypes.create_string_buffer(m, max(1, len(m))) for m in msgs]
        outs = [ctypes.create_string_buffer(FILL, 64) for _ in msgs]
        assert L.fd_sha512_gpu_batch_init(self.b) == self.b
        for m, buf, o in zip(msgs, bufs, outs):
            assert L.fd_sha512_gpu_batch_add(self.b, buf, len(m), o) == self.b
        return bufs, outs

    def run(self, msgs):
        bufs, outs = self.queue(msgs)
        assert self.L.fd_sha512_gpu_batch_fini(self.b) == self.b, fa.last_error()
        return [o.raw for o in outs]

    def check(self, msgs):
        hsz = 48 if self.is384 else 64
        got = self.run(msgs)
        for i, (m, g) in enumerate(zip(msgs, got)):
            assert g[:hsz] == expect(m, self.is384), (i, len(m))
            assert g[hsz:] == FILL[hsz:], (i, len(m))          # SHA-384 writes 48 bytes and no more

    def close(self):
        self.L.fd_sha512_gpu_batch_delete(self.b)


@pytest.fixture(scope="module")
def small():
    e = fa.Engine(0, 64, BLOB, depth=2)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[False, True], ids=["sha512", "sha384"])
def batch(request, small):
    b = Batch(small, request.param)
    yield b
    b.close()


@pytest.fixture(scope="module")
def tails():
    """every tail residue past the blob: 2,049 .. 2,176 bytes"""
    return rand_msgs(range(BLOB + 1, BLOB + 129), 11)


def mixed_msgs():
    sizes = [0, 1, 111, 112, 127, 128, BLOB, BLOB + 1, 2049, 5000, 40000]
    msgs = rand_msgs(sizes, 12)
    order = np.random.default_rng(13).permutation(len(msgs))
    return [msgs[i] for i in order]


def test_every_tail_alone(batch, tails):
    """m = 1: the largest C, every position of the padding bit and the count"""
    G, C = fa.sha512_long_geometry(BLOB, 64, 1)
    assert all(len(m) > C * 128 for m in tails)                # more than one launch each
    for m in tails:
        batch.check([m])


def test_every_tail_one_fini(batch, tails):
    G, _ = fa.sha512_long_geometry(BLOB, 64, 1)
    assert len(tails) > 2 * G                                  # several groups
    batch.check(tails)


def test_mixed_fini(batch, ref):
    """packed and long messages in one fini, queued shuffled: lanes finish at
    different launches (idle nblk == 0 lanes beside live ones), the 40,000
    byte message reuses the buffer dozens of times, every digest lands at its
    own pointer"""
    msgs = mixed_msgs()
    G, _ = fa.sha512_long_geometry(BLOB, 64, 1)
    nlong = sum(len(m) > BLOB for m in msgs)
    assert 1 < nlong <= G                                      # the long ones share one group
    _, C = fa.sha512_long_geometry(BLOB, 64, nlong)
    assert 40000 // (C * 128) >= 2 * 24                        # dozens of launches, also where the blob is two halves
    batch.check(msgs)
    for m in msgs:
        assert ref_hash(ref, m, batch.is384) == expect(m, batch.is384)


@pytest.mark.parametrize("groups", ["G", "G+1", "2G+1"])
def test_group_edges(batch, groups):
    G, _ = fa.sha512_long_geometry(BLOB, 64, 1)
    n = {"G": G, "G+1": G + 1, "2G+1": 2 * G + 1}[groups]
    rng = np.random.default_rng(14)
    batch.check(rand_msgs(BLOB + 1 + rng.integers(0, 3000, n), 15))


def test_second_wavefront():
    """a group wider than one wave: lane 64 and up get their own digests"""
    blob = next(b for b in range(144, 1 << 16, 16) if fa.sha512_long_geometry(b, 128, 1)[0] >= 65)
    G, _ = fa.sha512_long_geometry(blob, 128, 1)
    assert G >= 65 and fa.sha512_long_geometry(blob - 16, 128, 1)[0] < 65
    eng = fa.Engine(0, 128, blob, depth=2)
    try:
        for is384 in (False, True):
            b = Batch(eng, is384)
            for n in sorted({65, G}):
                rng = np.random.default_rng(16 + n)
                b.check(rand_msgs(blob + rng.integers(1, 3 * 128 + 1, n), 17))     # 1-3 blocks past the blob
            b.close()
    finally:
        eng.close()


def test_blob_no_multiple_of_128():
    eng = fa.Engine(0, 16, 3000)
    try:
        for is384 in (False, True):
            b = Batch(eng, is384)
            rng = np.random.default_rng(18)
            b.check(rand_msgs(3001 + rng.integers(0, 6000, 17), 19))
            b.close()
    finally:
        eng.close()


def test_acceptance_1mib_engine(ref):
    """0 B, 1 KB, 3 MB and 5 MB in one fini on a 1 MiB-blob engine"""
    eng = fa.Engine(0, 64, 1 << 20)
    msgs = rand_msgs([0, 1000, 3_000_000, 5_000_000], 20)
    try:
        for is384 in (False, True):
            b = Batch(eng, is384)
            b.check(msgs)
            b.close()
            for m in msgs:
                assert ref_hash(ref, m, is384) == expect(m, is384)
    finally:
        eng.close()


def test_abort_then_reuse(batch):
    L = fa.lib()
    long_m, short_m = rand_msgs([5000, 300], 21)
    _, outs = batch.queue([long_m])
    assert L.fd_sha512_gpu_batch_abort(batch.b) == batch.b
    assert L.fd_sha512_gpu_batch_fini(batch.b) == batch.b      # nothing queued: nothing written
    assert outs[0].raw == FILL
    for _ in range(2):
        batch.check([long_m, short_m])


def test_two_callers_one_engine(small):
    """two threads, each with its own batch object, each 2G long messages on
    the depth-2 engine: each takes a slot of its own for its groups"""
    G, _ = fa.sha512_long_geometry(BLOB, 64, 1)
    old = small.timeout_ns
    small.timeout_ns = 20_000_000_000
    errs = []

    def work(k):
        try:
            for is384 in (False, True):
                b = Batch(small, is384)
                rng = np.random.default_rng(30 + k)
                b.check(rand_msgs(BLOB + 1 + rng.integers(0, 4000, 2 * G), 40 + k))
                b.close()
        except BaseException as e:           # noqa: BLE001 (reported by the main thread)
            errs.append((k, repr(e)))

    th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(60)
    small.timeout_ns = old
    assert not any(t.is_alive() for t in th), "a caller did not return"
    assert not errs, errs


@pytest.mark.parametrize("is384", [False, True], ids=["sha512", "sha384"])
def test_pointer_entry(small, is384):
    msgs = mixed_msgs()
    assert small.sha512_any(msgs, is384=is384) == [expect(m, is384) for m in msgs]
    assert small.sha512_any([], is384=is384) == []
    with pytest.raises(fa.EngineError):                        # the packed entry keeps its limit
        small.sha512([m for m in msgs if len(m) > BLOB], is384=is384)
