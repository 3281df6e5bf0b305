"""Merkle trees on the host (include/fd_bmtree_gpu.h, fd_bmtree_host.c): the
model against the reference's vectors, then the commit interface, hash_leaf
and fd_bmtree_roots_batch against the model."""
import functools

import numpy as np
import pytest

import bmtree_grid as bg
import firedancer_amd as fa
from conftest import P


@functools.lru_cache(maxsize=None)
def _leaf_nodes(W):
    rng = np.random.default_rng(20 + W)
    return [bg.leaf(rng.bytes(int(rng.integers(0, 90))), W) for _ in range(300)]


def test_model_matches_reference_vectors():
    v = bg.vectors()
    for count, want in v["bmtree20"]["roots"].items():
        assert bg.root_of_nodes(bg.v20_nodes(int(count)), 20).hex() == want, count
    words = [w.encode() for w in v["bmtree32"]["leaves"]]
    assert len(words) == 11
    assert bg.root(words, 32).hex() == v["bmtree32"]["root"]


@pytest.mark.parametrize("W", [20, 32])
def test_commit_every_count_in_uneven_pieces(W):
    nodes = _leaf_nodes(W)
    pieces = [1, 2, 7, 3, 16, 1, 31, 5]
    for count in range(1, 301):
        c = fa.BmtreeCommit(W)
        assert c.leaf_cnt == 0
        at, k = 0, 0
        while at < count:
            take = min(pieces[k % len(pieces)], count - at)
            assert c.append(nodes[at:at + take]) is c
            at += take
            k += 1
            assert c.leaf_cnt == at
        assert c.fini() == bg.root_of_nodes(nodes[:count], W), count
        assert c.leaf_cnt == count


def test_commit_reference_vectors():
    v = bg.vectors()
    for count in (1, 2, 3, 10):
        c = fa.BmtreeCommit(20)
        c.append([x.tobytes() for x in bg.v20_nodes(count)])
        assert c.fini().hex() == v["bmtree20"]["roots"][str(count)]
    c = fa.BmtreeCommit(32)
    c.append([fa.bmtree_hash_leaf(32, w.encode()) for w in v["bmtree32"]["leaves"]])
    assert c.fini().hex() == v["bmtree32"]["root"]


def test_roots_batch_million_leaf_vector():
    nodes = bg.v20_nodes(1000000)
    leaves = np.zeros(1000000, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = np.arange(1000000, dtype=np.uint32) * 20
    leaves["sz"] = 20
    roots, codes = fa.bmtree_roots_batch(20, [1000000], leaves, nodes.reshape(-1), 1000000, fa.BMTREE_LEAVES_ARE_NODES, nthreads=1)
    assert codes[0] == 0
    assert roots[0, :20].tobytes().hex() == bg.vectors()["bmtree20"]["roots"]["1000000"]
    assert not roots[0, 20:].any()


@pytest.mark.parametrize("W", [20, 32])
def test_hash_leaf_every_size(W):
    rng = np.random.default_rng(3)
    for sz in range(201):
        d = rng.bytes(sz)
        assert fa.bmtree_hash_leaf(W, d) == bg.leaf(d, W), sz


def test_sizeof_and_align():
    L = fa.lib()
    for w in ("20", "32"):
        assert getattr(L, f"fd_bmtree{w}_commit_align")() == 32
        assert getattr(L, f"fd_bmtree{w}_commit_footprint")() == 2048


@pytest.mark.parametrize("nthreads", [1, 5])
@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_roots_batch_with_every_refusal(W, nodes, nthreads):
    cnt, leaves, blob, leaf_max, bad = bg.refusal_batch(W, nodes)
    want_r, want_c = bg.model(W, cnt, leaves, blob, leaf_max, nodes)
    assert sorted(np.nonzero(want_c)[0].tolist()) == bad
    got_r, got_c = fa.bmtree_roots_batch(W, cnt, leaves, blob, leaf_max, fa.BMTREE_LEAVES_ARE_NODES if nodes else 0, nthreads)
    assert (got_c == want_c).all()
    assert (got_r == want_r).all()
    assert not got_r[bad].any()


@pytest.mark.parametrize("nthreads", [1, 5])
@pytest.mark.parametrize("W", [20, 32])
def test_roots_batch_grid(W, nthreads):
    counts = list(range(1, 70)) + [127, 128, 129, 300]
    cnt, leaves, blob = bg.sig_batch(counts, 5)
    want_r, want_c = bg.model(W, cnt, leaves, blob, 300)
    got_r, got_c = fa.bmtree_roots_batch(W, cnt, leaves, blob, 300, 0, nthreads)
    assert (got_c == 0).all() and (want_c == 0).all()
    assert (got_r == want_r).all()


@pytest.mark.parametrize("T", [257, 1279])
@pytest.mark.parametrize("W", [20, 32])
def test_roots_batch_blocks_of_trees(W, T):
    """the device tests' batches around the set-up blocks of 256 trees
    (tests/test_gpu_bmtree_blocks.py), so that the yardstick is held to the
    model on them too"""
    for name in bg.block_variants(T):
        cnt, leaves, blob = bg.block_batch(T, name)
        want_r, want_c = bg.model(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX)
        assert ((want_c != 0) == ((cnt == 0) | (cnt == 34))).all()
        got_r, got_c = fa.bmtree_roots_batch(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX, 0, 5)
        assert (got_c == want_c).all() and (got_r == want_r).all(), name


@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_roots_batch_tight_shapes(W, nodes):
    """the shapes that meet the device call's lane bound and capacities"""
    for k, counts in enumerate(bg.TIGHT_SHAPES):
        cnt, leaves, blob = bg.tight_batch(counts, W, nodes, 600 + k)
        for leaf_max in (max(counts), 1 << 30):
            want_r, want_c = bg.model(W, cnt, leaves, blob, leaf_max, nodes)
            got_r, got_c = fa.bmtree_roots_batch(W, cnt, leaves, blob, leaf_max, fa.BMTREE_LEAVES_ARE_NODES if nodes else 0, 3)
            assert (want_c == 0).all() and (got_c == 0).all() and (got_r == want_r).all(), counts[:3]


@pytest.mark.parametrize("nodes", [False, True])
def test_model_refusals_rule_by_rule(nodes):
    """the model's vectorised refusals against bg.refused, the header's rules one descriptor at a time"""
    cnt, leaves, blob, leaf_max, bad = bg.refusal_batch(32, nodes)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    slow = [bg.refused(int(c), [(int(d["off"]), int(d["sz"])) for d in leaves[first[t]:first[t + 1]]], len(blob), leaf_max, 32, nodes)
            for t, c in enumerate(cnt)]
    assert np.nonzero(slow)[0].tolist() == bad
    assert ((bg.model(32, cnt, leaves, blob, leaf_max, nodes)[1] != 0) == slow).all()


def test_layer_helpers():
    """bmtree_grid's shape helpers on cases done by hand"""
    assert bg.layer_counts([5, 1, 0, 3], 5) == [3 + 2, 2 + 1, 1]
    assert bg.layer_counts([5, 1, 0, 3], 4) == [2, 1]
    assert bg.layer_counts([1, 0], 8) == []
    assert bg.layer_bound(3, 15, 2) == 6 and bg.layer_bound(1, 3, 1) == 2 and bg.layer_bound(3, 35, 6) == 1
    cnt, leaves, blob = bg.pool_batch([2, 0, 3], 20, 1)
    assert blob.nbytes == 4096 * 20 and (leaves["sz"] == 20).all() and (leaves["off"] % 20 == 0).all() and len(leaves) == 5
    assert len(set(leaves["off"].tolist())) == 5


def test_roots_batch_bad_calls():
    L = fa.lib()
    cnt, leaves, blob = bg.sig_batch([2, 3], 6)
    roots = np.full((2, 32), 0x55, np.uint8)
    codes = np.full(2, 77, np.int32)
    args = lambda **k: [k.get("w", 32), k.get("f", 0), 2, k.get("cnt", P(cnt)), P(leaves), P(blob), blob.nbytes, 8,  # noqa: E731
                        k.get("r", P(roots)), P(codes), k.get("th", 1)]
    assert L.fd_bmtree_roots_batch(*args(w=24)) == fa.ERR_ARG
    assert L.fd_bmtree_roots_batch(*args(f=2)) == fa.ERR_ARG
    assert L.fd_bmtree_roots_batch(*args(cnt=None)) == fa.ERR_ARG
    assert L.fd_bmtree_roots_batch(*args(r=None)) == fa.ERR_ARG
    assert L.fd_bmtree_roots_batch(*args(th=0)) == fa.ERR_ARG
    assert L.fd_bmtree_roots_batch(*args(th=257)) == fa.ERR_ARG
    assert (roots == 0x55).all() and (codes == 77).all()
    assert L.fd_bmtree_roots_batch(*args()) == 0
    assert (codes == 0).all()


def test_merge_passes_counted_from_shapes():
    # 65 trees of 2 leaves: 65 parents, two waves; width 32 merges are two blocks each
    assert fa.bmtree_merge_passes(20, [2] * 65) == 2
    assert fa.bmtree_merge_passes(32, [2] * 65) == 4
    # one tree of 5: layers of 3, 2, 1 parents, a wave each; single leaves and empty trees merge nothing
    assert fa.bmtree_merge_passes(20, [5, 1, 0]) == 3
