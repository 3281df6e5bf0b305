"""Proof-of-History chains on the device (fd_k_poh through
Engine.poh_verify and Engine.poh_verify_dev): every code and every final
state against hashlib.sha256.  Launch boundaries are crossed with tiny
chains through the debug chunk knob.

Mainnet block 1 runs whole, as seven entries: its longest lane (428,775
hashes) measured 1.16 s on an MI355X, under the 5 s above which it would
have been cut to its first two entries."""
import functools
import time

import numpy as np
import pytest

import firedancer_amd as fa
import poh_grid as pg
from conftest import P, load_corpus, oracle_batch

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 130]
CHUNKS = [1, 4, 64]


@functools.lru_cache(maxsize=None)
def _grid(C, count):
    return pg.grid(C, count)


@pytest.fixture
def chunk(engine):
    """sets the hashes per launch for one test and puts the default back"""
    def set_(C):
        engine.poh_chunk = C
    yield set_
    engine.poh_chunk = 0
    assert engine.poh_chunk == fa.POH_CHUNK_DEFAULT


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("count", COUNTS)
def test_grid_packed(engine, chunk, C, count):
    ent, codes, states = _grid(C, count)
    chunk(C)
    got, st = engine.poh_verify(ent, 2 * C + 1, states=True)
    assert (got == codes).all()
    assert (st == states).all()
    assert (engine.poh_verify(ent, 2 * C + 1) == codes).all()


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("own_stream", [False, True])
def test_grid_dev_caller_order(engine, chunk, C, count, own_stream):
    import torch
    ent, codes, states = _grid(C, count)
    chunk(C)
    dev = torch.device("cuda", 0)
    d_ent = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
    d_out = torch.full((count,), 77, dtype=torch.int32, device=dev)
    d_st = torch.full((count, 32), 0x55, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(fa.poh_work_sz(count), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if own_stream:
        stream = torch.cuda.Stream(dev)
        engine.poh_verify_dev(count, d_ent.data_ptr(), 2 * C + 1, d_out.data_ptr(), d_st.data_ptr(), d_work.data_ptr(),
                              stream.cuda_stream)
        stream.synchronize()
    else:
        engine.poh_verify_dev(count, d_ent.data_ptr(), 2 * C + 1, d_out.data_ptr(), d_st.data_ptr(), d_work.data_ptr())
        torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == codes).all()
    assert (d_st.cpu().numpy() == states).all()
    # without states; n_max far past every chain: the extra launches find every row done
    d_out.fill_(77)
    torch.cuda.synchronize()
    engine.poh_verify_dev(count, d_ent.data_ptr(), 20 * C, d_out.data_ptr(), 0, d_work.data_ptr())
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == codes).all()


def test_default_chunk(engine):
    assert engine.poh_chunk == fa.POH_CHUNK_DEFAULT == 16384
    rng = np.random.default_rng(8)
    ns = [16383, 16384, 16385]
    ent = np.zeros(3, fa.POH_ENTRY_DTYPE)
    for i, n in enumerate(ns):
        pg.entry(ent[i], rng.bytes(32), n, rng.bytes(32))
    got, st = engine.poh_verify(ent, 16385, states=True)
    assert (got == 0).all()
    assert (st == ent["expect"]).all()


def test_wrong_expect_and_unread_mixin(engine, chunk):
    chunk(4)
    rng = np.random.default_rng(9)
    ent = np.zeros(70, fa.POH_ENTRY_DTYPE)
    for i in range(70):
        pg.entry(ent[i], rng.bytes(32), i % 11, rng.bytes(32) if i % 3 == 0 else None)
    true = ent["expect"].copy()
    exp = np.zeros(70, np.int32)
    for i, byte in ((0, 0), (1, 15), (2, 31), (66, 0), (67, 15), (68, 31)):
        ent[i]["expect"][byte] ^= 1 << (i % 8)
        exp[i] = fa.POH_ERR_HASH
    got, st = engine.poh_verify(ent, 10, states=True)
    assert (got == exp).all()
    assert (st == true).all()                    # the true state, also where expect is wrong
    for i in range(70):                          # garbage in mixin with the flag clear changes nothing
        if not ent[i]["flags"]:
            ent[i]["mixin"] = np.frombuffer(rng.bytes(32), np.uint8)
    got2, st2 = engine.poh_verify(ent, 10, states=True)
    assert (got2 == exp).all() and (st2 == true).all()


def test_err_arg_entries(engine, chunk):
    chunk(4)
    rng = np.random.default_rng(10)
    ent = np.zeros(67, fa.POH_ENTRY_DTYPE)
    for i in range(67):
        pg.entry(ent[i], rng.bytes(32), (i * 5) % 9 if i % 4 else 0, rng.bytes(32) if i & 1 else None)
    true = ent["expect"].copy()
    exp = np.zeros(67, np.int32)
    ent[3]["flags"] |= 2
    ent[20]["_pad"] = 1
    ent[41]["n"] = 9                              # > n_max
    ent[63]["flags"] = 0x80000001
    ent[64]["n"] = 1 << 40
    for i in (3, 20, 41, 63, 64):
        exp[i], true[i] = fa.ERR_ARG, 0
    got, st = engine.poh_verify(ent, 8, states=True)
    assert (got == exp).all()                     # the neighbours, n = 0 among them, are unaffected
    assert (st == true).all()
    host, hst = fa.poh_verify_batch(ent, 8, states=True)
    assert (host == exp).all() and (hst == true).all()
    # only n = 0 entries: one launch, return value 0, every code written
    z = np.zeros(5, fa.POH_ENTRY_DTYPE)
    for i in range(5):
        pg.entry(z[i], rng.bytes(32), 0, rng.bytes(32) if i & 1 else None)
    assert (engine.poh_verify(z, 0) == 0).all()


def test_order_independence(engine, chunk):
    chunk(4)
    ent, codes, states = _grid(4, 130)
    perm = np.random.default_rng(12).permutation(130)
    got, st = engine.poh_verify(ent[perm], 9, states=True)
    assert (got == codes[perm]).all()
    assert (st == states[perm]).all()


def test_large_count_and_scratch_growth():
    """70,000 entries from an engine whose PoH scratch was sized by a
    64-entry call"""
    e = fa.Engine(0, 1 << 10, 1 << 16)
    try:
        rng = np.random.default_rng(13)
        n = 70000
        ent = np.zeros(n, fa.POH_ENTRY_DTYPE)
        ent["start"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ent["mixin"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ent["n"] = rng.integers(0, 4, n)
        ent["flags"] = rng.integers(0, 2, n)
        states = np.zeros((n, 32), np.uint8)
        for i in range(n):
            mx = ent["mixin"][i].tobytes() if ent["flags"][i] else None
            states[i] = np.frombuffer(pg.ref(ent["start"][i].tobytes(), int(ent["n"][i]), mx), np.uint8)
        ent["expect"] = states
        bad = rng.choice(n, 200, replace=False)
        ent["expect"][bad, 7] ^= 0x80
        exp = np.zeros(n, np.int32)
        exp[bad] = fa.POH_ERR_HASH
        got, st = e.poh_verify(ent[:64], 3, states=True)
        assert (got == exp[:64]).all() and (st == states[:64]).all()
        e.poh_chunk = 2
        got, st = e.poh_verify(ent, 3, states=True)
        assert (got == exp).all()
        assert (st == states).all()
    finally:
        e.close()


def test_block1_as_seven_entries(engine):
    ent, post = pg.block1_entries()
    t0 = time.perf_counter()
    got, st = engine.poh_verify(ent, 428775, states=True)
    dt = time.perf_counter() - t0
    print(f"block 1, seven entries, longest lane 428,775 hashes: {dt:.3f} s")
    assert (got == 0).all()
    assert (st == ent["expect"]).all()
    assert st[-1].tobytes() == post


def test_timeout_writes_nothing_and_engine_recovers(oracle):
    e = fa.Engine(0, 1 << 13, 1 << 21)            # holds the adversarial corpus (6,144 signatures, 1.4 MB)
    try:
        rng = np.random.default_rng(14)
        n_hash = 40000
        ent = np.zeros(64, fa.POH_ENTRY_DTYPE)
        start = rng.bytes(32)
        pg.entry(ent[0], start, n_hash, None)
        for i in range(1, 64):
            ent[i] = ent[0]
        e.poh_chunk = 64                          # 625 launches
        out = np.full(64, 77, np.int32)
        st = np.full((64, 32), 0x55, np.uint8)
        e.timeout_ns = 1_000_000
        r = fa.lib().fd_poh_gpu_verify_packed(e._h, 64, P(ent), n_hash, P(out), P(st))
        assert r == fa.ERR_GPU
        assert "not complete" in fa.last_error()
        assert (out == 77).all() and (st == 0x55).all()
        e.timeout_ns = 10_000_000_000
        b, _ = load_corpus("adversarial")
        assert (e.verify_packed(b.blob, b.desc) == oracle_batch(oracle, b)).all()
        got, st2 = e.poh_verify(ent, n_hash, states=True)   # waits for the abandoned launches first
        assert (got == 0).all() and (st2 == ent["expect"]).all()
    finally:
        e.close()
