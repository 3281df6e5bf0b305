"""Merkle roots on the device (fd_k_bmtree_* through Engine.bmtree_roots and
Engine.bmtree_roots_dev): every root and every code against the model of
tests/bmtree_grid.py (hashlib, layer by layer) and the reference's vectors."""
import functools

import numpy as np
import pytest

import bmtree_grid as bg
import firedancer_amd as fa
from conftest import P

pytestmark = pytest.mark.gpu

COUNTS = list(range(1, 131)) + [255, 256, 257, 4095, 4096, 4097]
SIZES = list(range(0, 131)) + [1203, 1228]
NODES = fa.BMTREE_LEAVES_ARE_NODES


@functools.lru_cache(maxsize=None)
def _count_grid(W):
    """every count of COUNTS once, shuffled, 64-byte leaves; with the model's roots"""
    order = np.random.default_rng(100 + W).permutation(len(COUNTS))
    cnt, leaves, blob = bg.sig_batch([COUNTS[i] for i in order], 200 + W)
    roots, codes = bg.model(W, cnt, leaves, blob, 4097)
    assert (codes == 0).all()
    return cnt, leaves, blob, roots


@functools.lru_cache(maxsize=None)
def _size_grid(W):
    """three-leaf trees: leaf sizes SIZES, the k-th leaf starting at k mod 16,
    the last leaf ending exactly at blob_sz"""
    rng = np.random.default_rng(300 + W)
    trees = [[rng.bytes(s), rng.bytes(SIZES[(i + 7) % len(SIZES)]), rng.bytes(s)] for i, s in enumerate(SIZES)]
    cnt, leaves, blob = bg.pack(trees, align_of=lambda k: k)
    assert int(leaves[-1]["off"]) + int(leaves[-1]["sz"]) == len(blob)
    assert sorted(set((leaves["off"] % 16).tolist())) == list(range(16))
    roots, codes = bg.model(W, cnt, leaves, blob, 3)
    assert (codes == 0).all()
    return cnt, leaves, blob, roots


@pytest.mark.parametrize("W", [20, 32])
def test_every_count_in_one_shuffled_call(engine, W):
    cnt, leaves, blob, want = _count_grid(W)
    roots, codes = engine.bmtree_roots(W, cnt, leaves, blob, 4097)
    assert (codes == 0).all()
    assert (roots == want).all()
    if W == 20:
        assert not roots[:, 20:].any()


@pytest.mark.parametrize("W", [20, 32])
def test_leaf_sizes_and_alignments(engine, W):
    cnt, leaves, blob, want = _size_grid(W)
    roots, codes = engine.bmtree_roots(W, cnt, leaves, blob, 3)
    assert (codes == 0).all()
    assert (roots == want).all()


def _node_leaves(count, W):
    leaves = np.zeros(count, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = np.arange(count, dtype=np.uint32) * W
    leaves["sz"] = W
    return leaves


def test_golden_vectors_node_mode(engine):
    v = bg.vectors()
    counts = [int(c) for c in v["bmtree20"]["roots"]]
    assert 1000000 in counts
    # all five trees in one call: tree k's nodes are le64(0..count-1), so they share the blob
    blob = bg.v20_nodes(max(counts)).reshape(-1)
    leaves = np.concatenate([_node_leaves(c, 20) for c in counts])
    roots, codes = engine.bmtree_roots(20, counts, leaves, blob, max(counts), NODES)
    assert (codes == 0).all()
    for k, c in enumerate(counts):
        assert roots[k, :20].tobytes().hex() == v["bmtree20"]["roots"][str(c)], c
    assert not roots[:, 20:].any()
    # the 32-byte vector: as words through the leaf hash, and as ready nodes
    words = [w.encode() for w in v["bmtree32"]["leaves"]]
    cnt, lv, bl = bg.pack([words])
    roots, codes = engine.bmtree_roots(32, cnt, lv, bl, 11)
    assert codes[0] == 0 and roots[0].tobytes().hex() == v["bmtree32"]["root"]
    nodes = np.frombuffer(b"".join(bg.leaf(w, 32) for w in words), np.uint8)
    roots, codes = engine.bmtree_roots(32, [11], _node_leaves(11, 32), nodes, 11, NODES)
    assert codes[0] == 0 and roots[0].tobytes().hex() == v["bmtree32"]["root"]


@pytest.mark.parametrize("W", [20, 32])
def test_one_leaf_tree_is_its_leaf(engine, W):
    rng = np.random.default_rng(5)
    node = rng.integers(1, 256, W, dtype=np.uint8)
    roots, codes = engine.bmtree_roots(W, [1], _node_leaves(1, W), node, 1, NODES)
    assert codes[0] == 0
    assert (roots[0, :W] == node).all() and not roots[0, W:].any()
    data = rng.integers(0, 256, 64, dtype=np.uint8)
    lv = np.array([(0, 64)], fa.BMTREE_LEAF_DTYPE)
    roots, codes = engine.bmtree_roots(W, [1], lv, data, 1)       # hashed once, not again
    assert codes[0] == 0
    assert roots[0, :W].tobytes() == bg.leaf(data.tobytes(), W) and not roots[0, W:].any()


@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_every_refusal_between_valid_trees(engine, W, nodes):
    cnt, leaves, blob, leaf_max, bad = bg.refusal_batch(W, nodes)
    want_r, want_c = bg.model(W, cnt, leaves, blob, leaf_max, nodes)
    assert sorted(np.nonzero(want_c)[0].tolist()) == bad
    roots, codes = engine.bmtree_roots(W, cnt, leaves, blob, leaf_max, NODES if nodes else 0)
    assert (codes == want_c).all()
    assert (roots == want_r).all()
    assert not roots[bad].any()
    host_r, host_c = fa.bmtree_roots_batch(W, cnt, leaves, blob, leaf_max, NODES if nodes else 0)
    assert (host_c == want_c).all() and (host_r == want_r).all()


def test_only_refused_trees_and_empty_calls(engine):
    z = np.zeros(0, fa.BMTREE_LEAF_DTYPE)
    roots, codes = engine.bmtree_roots(32, [0, 0, 0], z, np.zeros(0, np.uint8), 4)
    assert (codes == fa.ERR_ARG).all() and not roots.any()
    roots, codes = engine.bmtree_roots(32, [], z, np.zeros(0, np.uint8), 4)
    assert len(roots) == 0 and len(codes) == 0


@pytest.mark.parametrize("W", [20, 32])
def test_one_flipped_bit(engine, W):
    counts = [1 + (7 * i) % 23 for i in range(40)]
    cnt, leaves, blob = bg.sig_batch(counts, 9)
    base, _ = engine.bmtree_roots(W, cnt, leaves, blob, 23)
    rng = np.random.default_rng(10)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    flipped = blob.copy()
    for t in range(40):
        k = first[t] + int(rng.integers(counts[t]))
        flipped[64 * k + int(rng.integers(64))] ^= 1 << int(rng.integers(8))
    want, _ = bg.model(W, cnt, leaves, flipped, 23)
    got, codes = engine.bmtree_roots(W, cnt, leaves, flipped, 23)
    assert (codes == 0).all()
    assert (got == want).all()
    assert (got != base).any(axis=1).all()                        # every tree's root moved


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_dev_strided_roots_into_sentinels(engine, W, own_stream):
    import torch
    cnt, leaves, blob, want = _count_grid(W)
    T, N = len(cnt), len(leaves)
    dev = torch.device("cuda", 0)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_roots = torch.full((T, 112), 0x5A, dtype=torch.uint8, device=dev)
    d_codes = torch.full((T,), 77, dtype=torch.int32, device=dev)
    d_work = torch.zeros(fa.bmtree_work_sz(T, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (W, T, d_first.data_ptr(), N, d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, 4097, d_roots.data_ptr() + 32, 112,
            d_codes.data_ptr(), d_work.data_ptr())
    if own_stream:
        stream = torch.cuda.Stream(dev)
        engine.bmtree_roots_dev(*args, stream.cuda_stream)
        stream.synchronize()
    else:
        engine.bmtree_roots_dev(*args)
        torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    got = d_roots.cpu().numpy()
    assert (got[:, 32:64] == want).all()
    assert (got[:, :32] == 0x5A).all() and (got[:, 64:] == 0x5A).all()      # every other byte untouched
    # leaf_max far past every tree: the extra launches find nothing to do
    d_roots.fill_(0x5A)
    d_codes.fill_(77)
    torch.cuda.synchronize()
    engine.bmtree_roots_dev(*args[:7], 1 << 30, *args[8:])
    torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    assert (d_roots.cpu().numpy()[:, 32:64] == want).all()


def test_scratch_growth_and_second_engine():
    """a large call after a small one on an engine of its own"""
    e = fa.Engine(0, 1 << 10, 1 << 16)
    try:
        cnt, leaves, blob = bg.sig_batch([3, 1, 2], 11)
        want, _ = bg.model(32, cnt, leaves, blob, 3)
        got, codes = e.bmtree_roots(32, cnt, leaves, blob, 3)
        assert (codes == 0).all() and (got == want).all()
        cnt, leaves, blob, want = _count_grid(32)
        got, codes = e.bmtree_roots(32, cnt, leaves, blob, 4097)
        assert (codes == 0).all() and (got == want).all()
    finally:
        e.close()


def test_timeout_writes_nothing_and_engine_recovers():
    """a packed call that gives up waiting writes nothing, and the next one
    waits the abandoned launches out before it uses the scratch"""
    e = fa.Engine(0, 1 << 10, 1 << 16)
    try:
        cnt, leaves, blob = bg.sig_batch([16] * 4096, 12)        # 65,536 leaves, a 4 MiB blob
        want, want_codes = bg.model(32, cnt, leaves, blob, 16)
        assert (want_codes == 0).all()
        roots = np.full((4096, 32), 0x5A, np.uint8)
        codes = np.full(4096, 77, np.int32)
        e.timeout_ns = 1_000                                     # the 4 MiB copy alone takes some 65 us
        r = fa.lib().fd_bmtree_gpu_roots_packed(e._h, 32, 0, 4096, P(cnt), P(leaves), P(blob), blob.nbytes, 16, P(roots), P(codes))
        assert r == fa.ERR_GPU
        assert "not complete" in fa.last_error()
        assert (roots == 0x5A).all() and (codes == 77).all()
        e.timeout_ns = 10_000_000_000
        got, got_codes = e.bmtree_roots(32, cnt, leaves, blob, 16)
        assert (got_codes == 0).all() and (got == want).all()
        # a smaller call after a larger one on a unit that was busy
        cnt, leaves, blob = bg.sig_batch([3, 1, 2], 11)
        want, _ = bg.model(32, cnt, leaves, blob, 3)
        got, got_codes = e.bmtree_roots(32, cnt, leaves, blob, 3)
        assert (got_codes == 0).all() and (got == want).all()
    finally:
        e.close()
