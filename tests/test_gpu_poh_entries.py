"""Proof-of-History entries from leaves on the device
(Engine.poh_verify_entries and Engine.poh_verify_entries_dev): an entry with
leaves takes its mixin from the bmtree32 root of its leaves.  Codes and final
states must equal Engine.poh_verify on the same entries carrying the model's
roots (tests/bmtree_grid.py) as mixins, and hashlib's."""
import functools

import numpy as np
import pytest

import bmtree_grid as bg
import firedancer_amd as fa
import poh_grid as pg
from conftest import P

pytestmark = pytest.mark.gpu

CHUNKS = [1, 4, 64]
COUNT = 130


@pytest.fixture
def chunk(engine):
    def set_(C):
        engine.poh_chunk = C
    yield set_
    engine.poh_chunk = 0


@functools.lru_cache(maxsize=None)
def _batch(C):
    """130 entries cycling ticks, caller-mixin entries and leaf entries with
    0..9 leaves over poh_grid's lengths; every 7th expect has one bit wrong.
    Returns (entries for the entries call, the same with the model's roots
    as mixins, leaf_cnt, leaves, blob, codes, states)."""
    rng = np.random.default_rng(500 + C)
    lengths = pg.grid_lengths(C)
    trees, kinds = [], []
    for i in range(COUNT):
        kind = i % 3                                   # 0 tick, 1 caller's mixin, 2 leaves
        n_leaf = (i // 3) % 10 if kind == 2 else 0
        if kind == 2 and n_leaf == 0:
            kind = 1                                   # a leaf entry without leaves is a caller-mixin entry
        kinds.append(kind)
        trees.append([rng.bytes(64) for _ in range(n_leaf)])
    cnt, leaves, blob = bg.pack(trees, align_of=lambda k: 5 * k)   # signatures at any alignment, as inside payloads
    ent = np.zeros(COUNT, fa.POH_ENTRY_DTYPE)
    ref = np.zeros(COUNT, fa.POH_ENTRY_DTYPE)
    codes = np.zeros(COUNT, np.int32)
    states = np.zeros((COUNT, 32), np.uint8)
    for i in range(COUNT):
        n = lengths[(i * 5 + i // 9) % len(lengths)]
        start = rng.bytes(32)
        mixin = None if kinds[i] == 0 else rng.bytes(32) if kinds[i] == 1 else bg.root(trees[i], 32)
        pg.entry(ref[i], start, n, mixin)
        states[i] = ref[i]["expect"]
        if i % 7 == 3:
            ref[i]["expect"][int(rng.integers(32))] ^= 1 << int(rng.integers(8))
            codes[i] = fa.POH_ERR_HASH
        ent[i] = ref[i]
        if kinds[i] != 1:
            ent[i]["mixin"] = np.frombuffer(rng.bytes(32), np.uint8)   # garbage: unread (tick) or overwritten (leaves)
    assert set(cnt.tolist()) == set(range(10))
    return ent, ref, cnt, leaves, blob, codes, states


@pytest.mark.parametrize("C", CHUNKS)
def test_entries_packed(engine, chunk, C):
    ent, ref, cnt, leaves, blob, codes, states = _batch(C)
    chunk(C)
    want_c, want_s = engine.poh_verify(ref, 2 * C + 1, states=True)
    assert (want_c == codes).all() and (want_s == states).all()
    before = ent.copy()
    got_c, got_s = engine.poh_verify_entries(ent, 2 * C + 1, cnt, leaves, blob, 9, states=True)
    assert (got_c == want_c).all()
    assert (got_s == want_s).all()
    assert (ent == before).all()                       # the caller's entries are not written
    assert (engine.poh_verify_entries(ent, 2 * C + 1, cnt, leaves, blob, 9) == want_c).all()
    # no leaves at all: exactly poh_verify
    zero = np.zeros(COUNT, np.uint32)
    none = np.zeros(0, fa.BMTREE_LEAF_DTYPE)
    a, b = engine.poh_verify_entries(ref, 2 * C + 1, zero, none, blob, 9, states=True)
    assert (a == want_c).all() and (b == want_s).all()


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("own_stream", [False, True])
def test_entries_dev(engine, chunk, C, own_stream):
    import torch
    ent, ref, cnt, leaves, blob, codes, states = _batch(C)
    chunk(C)
    dev = torch.device("cuda", 0)
    N = len(leaves)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    d_ent = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_out = torch.full((COUNT,), 77, dtype=torch.int32, device=dev)
    d_st = torch.full((COUNT, 32), 0x55, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(fa.poh_work_sz(COUNT), dtype=torch.uint8, device=dev)
    d_twork = torch.zeros(fa.poh_entries_work_sz(COUNT, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (COUNT, d_ent.data_ptr(), 2 * C + 1, d_out.data_ptr(), d_st.data_ptr(), d_work.data_ptr(), d_first.data_ptr(), N,
            d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, 9, d_twork.data_ptr())
    if own_stream:
        stream = torch.cuda.Stream(dev)
        engine.poh_verify_entries_dev(*args, stream.cuda_stream)
        stream.synchronize()
    else:
        engine.poh_verify_entries_dev(*args)
        torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == codes).all()
    assert (d_st.cpu().numpy() == states).all()
    # the device copy: roots in the mixins of the leaf entries, everything else as it was
    after = d_ent.cpu().numpy().view(fa.POH_ENTRY_DTYPE)
    has = cnt > 0
    assert (after["mixin"][has] == ref["mixin"][has]).all()
    assert (after["mixin"][~has] == ent["mixin"][~has]).all()
    for f in ("start", "expect", "n", "flags", "_pad"):
        assert (after[f] == ent[f]).all(), f


def _small(rng, n_leaf_list, n_hash=None):
    trees = [[rng.bytes(64) for _ in range(k)] for k in n_leaf_list]
    cnt, leaves, blob = bg.pack(trees)
    ent = np.zeros(len(trees), fa.POH_ENTRY_DTYPE)
    for i, t in enumerate(trees):
        pg.entry(ent[i], rng.bytes(32), n_hash or 3 + i % 4, bg.root(t, 32) if t else (rng.bytes(32) if i & 1 else None))
    return trees, cnt, leaves, blob, ent


def test_one_signature_bit_wrong(engine, chunk):
    chunk(4)
    rng = np.random.default_rng(21)
    trees, cnt, leaves, blob, ent = _small(rng, [(i * 3) % 7 for i in range(70)])
    true = ent["expect"].copy()
    assert (engine.poh_verify_entries(ent, 6, cnt, leaves, blob, 6) == 0).all()
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    victim = 44
    assert cnt[victim] > 1
    bad = blob.copy()
    bad[int(leaves[first[victim] + 1]["off"]) + 17] ^= 0x10
    got, st = engine.poh_verify_entries(ent, 6, cnt, leaves, bad, 6, states=True)
    exp = np.zeros(70, np.int32)
    exp[victim] = fa.POH_ERR_HASH
    assert (got == exp).all()
    ok = np.arange(70) != victim
    assert (st[ok] == true[ok]).all() and (st[victim] != true[victim]).any()


def test_leaves_without_flag_refused_trees_and_n_max(engine, chunk):
    chunk(4)
    rng = np.random.default_rng(22)
    trees, cnt, leaves, blob, ent = _small(rng, [(i * 5) % 9 for i in range(67)])
    true = ent["expect"].copy()
    exp = np.zeros(67, np.int32)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    leaves = leaves.copy()
    over = np.nonzero(cnt == 8)[0].tolist()            # 8 leaves > leaf_max 7
    assert 0 < cnt[5] < 8 and 0 < cnt[23] < 8 and 0 < cnt[31] < 8 and cnt[9] == 0 and len(over) == 7
    ent[5]["flags"] = 0                                # leaves without FD_POH_GPU_MIXIN
    leaves[first[23]]["off"] = len(blob) - 10          # a leaf past the blob: its tree is refused
    ent[31]["n"] = 7                                   # > n_max, as in poh_verify
    ent[9]["flags"] |= 2                               # an unknown flag on an entry without leaves
    for i in [5, 23, 31, 9] + over:
        exp[i], true[i] = fa.ERR_ARG, 0
    got, st = engine.poh_verify_entries(ent, 6, cnt, leaves, blob, 7, states=True)
    assert (got == exp).all()                          # the neighbours are unaffected
    assert (st == true).all()


BIG = 1300
SPECIAL = {0: "tick", 255: "noflag", 256: "size", 511: "blob", 512: "n_max", 1299: "blob_last"}


@functools.lru_cache(maxsize=None)
def _big_batch():
    """1,300 entries, over six set-up blocks of 256 trees and six blocks of
    the gate kernel, kinds and leaf counts cycling as in _batch, chains of
    0..5 hashes, leaf_max 8 (so 9 leaves are refused), every 7th expect
    flipped.  At entries 0, 255, 256, 511, 512 and 1,299, the first and the
    last entry of a block: a tick, leaves without FD_POH_GPU_MIXIN, a tree
    refused by size, trees refused by a descriptor past the blob (on the
    first leaf, and on the call's last leaf), and n > n_max on an entry with
    leaves.  Returns (entries, the same as Engine.poh_verify must see them:
    the model's roots as mixins and _pad set where the gate sets it,
    leaf_cnt, leaves, blob, codes, states, roots, gated, the trees' codes)."""
    rng = np.random.default_rng(77)
    n_leaf_of = {"tick": 0, "noflag": 3, "size": 9, "blob": 4, "n_max": 4, "blob_last": 5}
    kinds, trees = [], []
    for i in range(BIG):
        kind = i % 3
        n_leaf = (i // 3) % 10 if kind == 2 else 0
        if kind == 2 and n_leaf == 0:
            kind = 1
        if i in SPECIAL:
            n_leaf = n_leaf_of[SPECIAL[i]]
            kind = 2 if n_leaf else 0
        kinds.append(kind)
        trees.append([rng.bytes(64) for _ in range(n_leaf)])
    cnt, leaves, blob = bg.pack(trees, align_of=lambda k: 5 * k)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    leaves[first[511]]["off"] = len(blob) - 10
    leaves[first[1300] - 1]["off"] = len(blob) - 63
    roots, tcodes = bg.model(32, cnt, leaves, blob, 8)
    ent = np.zeros(BIG, fa.POH_ENTRY_DTYPE)
    ref = np.zeros(BIG, fa.POH_ENTRY_DTYPE)
    codes = np.zeros(BIG, np.int32)
    states = np.zeros((BIG, 32), np.uint8)
    gated = np.zeros(BIG, bool)
    for i in range(BIG):
        n = (i * 5 + i // 9) % 6
        start = rng.bytes(32)
        mixin = None if kinds[i] == 0 else rng.bytes(32) if kinds[i] == 1 else roots[i].tobytes()
        pg.entry(ref[i], start, n, mixin)
        if i % 7 == 3:
            ref[i]["expect"][int(rng.integers(32))] ^= 1 << int(rng.integers(8))
        ent[i] = ref[i]
        if kinds[i] != 1:
            ent[i]["mixin"] = np.frombuffer(rng.bytes(32), np.uint8)
        if SPECIAL.get(i) == "noflag":
            ent[i]["flags"] = ref[i]["flags"] = 0
        if SPECIAL.get(i) == "n_max":
            ent[i]["n"] = ref[i]["n"] = 6
        gated[i] = cnt[i] > 0 and (tcodes[i] != 0 or not ent[i]["flags"] & fa.POH_MIXIN)
        if gated[i] or ent[i]["n"] > 5:
            codes[i] = fa.ERR_ARG                    # refused unhashed: the state stays zero
        else:
            states[i] = np.frombuffer(pg.ref(start, n, mixin), np.uint8)
            codes[i] = fa.POH_ERR_HASH if i % 7 == 3 else 0
    ref["_pad"][gated] = 1
    # the placement
    assert cnt[0] == 0 and not ent[0]["flags"] and codes[0] == 0
    assert cnt[255] == 3 and tcodes[255] == 0 and gated[255]
    assert cnt[256] == 9 and tcodes[256] != 0 and gated[256]
    assert 0 < cnt[511] <= 8 and tcodes[511] != 0 and 0 < cnt[1299] <= 8 and tcodes[1299] != 0
    assert 0 < cnt[512] <= 8 and tcodes[512] == 0 and not gated[512] and codes[512] == fa.ERR_ARG
    assert all(codes[i] == fa.ERR_ARG for i in SPECIAL if i) and set(cnt.tolist()) == set(range(10))
    assert set(ent["n"][~gated].tolist()) == set(range(7)) and (codes == fa.POH_ERR_HASH).sum() > 150
    return ent, ref, cnt, leaves, blob, codes, states, roots, gated, tcodes


def test_entries_across_blocks_packed(engine, chunk):
    ent, ref, cnt, leaves, blob, codes, states, _, _, _ = _big_batch()
    chunk(2)
    want_c, want_s = engine.poh_verify(ref, 5, states=True)
    assert (want_c == codes).all() and (want_s == states).all()
    before = ent.copy()
    got_c, got_s = engine.poh_verify_entries(ent, 5, cnt, leaves, blob, 8, states=True)
    assert (got_c == codes).all()
    assert (got_s == states).all()
    assert (ent == before).all()


def test_entries_across_blocks_dev(engine, chunk):
    import torch
    ent, ref, cnt, leaves, blob, codes, states, roots, gated, tcodes = _big_batch()
    chunk(2)
    dev = torch.device("cuda", 0)
    N = len(leaves)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    d_ent = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_out = torch.full((BIG,), 77, dtype=torch.int32, device=dev)
    d_st = torch.full((BIG, 32), 0x55, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(fa.poh_work_sz(BIG), dtype=torch.uint8, device=dev)
    d_twork = torch.zeros(fa.poh_entries_work_sz(BIG, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.poh_verify_entries_dev(BIG, d_ent.data_ptr(), 5, d_out.data_ptr(), d_st.data_ptr(), d_work.data_ptr(), d_first.data_ptr(), N,
                                  d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, 8, d_twork.data_ptr())
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == codes).all()
    assert (d_st.cpu().numpy() == states).all()
    # the device copy: the mixins of the entries without leaves as they were, the model's root in every
    # accepted tree's entry, the zero root of a refused tree, _pad where the gate refuses, nothing else
    after = d_ent.cpu().numpy().view(fa.POH_ENTRY_DTYPE)
    has, okt = cnt > 0, (cnt > 0) & (tcodes == 0)
    assert (after["mixin"][~has] == ent["mixin"][~has]).all()
    assert (after["mixin"][okt] == roots[okt]).all() and roots[okt].any(axis=1).all()
    assert not after["mixin"][has & ~okt].any()
    assert (after["_pad"] == gated).all()
    for f in ("start", "expect", "n", "flags"):
        assert (after[f] == ent[f]).all(), f


def test_timeout_then_recovery():
    """a packed entries call that gives up waiting writes nothing, and the
    next one waits the abandoned launches out before it uses the scratch"""
    e = fa.Engine(0, 1 << 10, 1 << 16)
    try:
        n_hash = 40000
        # one entry of three signature leaves, 64 times: the chain is hashed here once
        _, cnt, leaves, blob, ent = _small(np.random.default_rng(23), [3], n_hash)
        assert ent[0]["flags"] == fa.POH_MIXIN
        cnt, leaves, ent = np.repeat(cnt, 64), np.tile(leaves, 64), np.repeat(ent, 64)
        e.poh_chunk = 64                          # 625 launches behind the trees
        out = np.full(64, 77, np.int32)
        st = np.full((64, 32), 0x55, np.uint8)
        e.timeout_ns = 1_000_000
        r = fa.lib().fd_poh_gpu_verify_entries_packed(e._h, 64, P(ent), n_hash, P(out), P(st), P(cnt), P(leaves), P(blob),
                                                      blob.nbytes, 3)
        assert r == fa.ERR_GPU
        assert "not complete" in fa.last_error()
        assert (out == 77).all() and (st == 0x55).all()
        e.timeout_ns = 10_000_000_000
        got, st2 = e.poh_verify_entries(ent, n_hash, cnt, leaves, blob, 3, states=True)
        assert (got == 0).all() and (st2 == ent["expect"]).all()
    finally:
        e.close()
