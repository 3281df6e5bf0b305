"""The schedule around the Merkle hashing on the device (fd_k_bmtree_sums,
_scan, _offsets, _check, _leaf and the lane counts of the device call), at
the shapes where it takes another path: more than one set-up block of 256
trees, more than one scan chunk of 1,024 block sums, shapes that meet the
device call's lane bound and node capacities exactly, one odd lane in a wave
of 64-byte leaves, and the largest leaf.  Every root and every code is
compared with the model of tests/bmtree_grid.py (hashlib, layer by layer),
through Engine.bmtree_roots (lanes counted on the host) and
Engine.bmtree_roots_dev (lanes from the shapes alone)."""
import functools

import numpy as np
import pytest

import bmtree_grid as bg
import firedancer_amd as fa

pytestmark = pytest.mark.gpu

NODES = fa.BMTREE_LEAVES_ARE_NODES


def dev_roots(engine, W, cnt, leaves, blob, leaf_max, flags=0):
    """Engine.bmtree_roots_dev with the roots strided into 0x5A sentinels;
    returns (roots (T, 32), codes) after checking that no other byte moved"""
    import torch
    dev = torch.device("cuda", 0)
    T, N = len(cnt), len(leaves)
    first = np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]).astype(np.uint32)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(np.ascontiguousarray(leaves).view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(np.ascontiguousarray(blob, np.uint8).copy()).to(dev)
    d_roots = torch.full((T, 112), 0x5A, dtype=torch.uint8, device=dev)
    d_codes = torch.full((T,), 77, dtype=torch.int32, device=dev)
    d_work = torch.zeros(fa.bmtree_work_sz(T, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.bmtree_roots_dev(W, T, d_first.data_ptr(), N, d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, leaf_max,
                            d_roots.data_ptr() + 32, 112, d_codes.data_ptr(), d_work.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    got = d_roots.cpu().numpy()
    assert (got[:, :32] == 0x5A).all() and (got[:, 64:] == 0x5A).all()
    return got[:, 32:64], d_codes.cpu().numpy()


def same(got, want):
    (roots, codes), (want_r, want_c) = got, want
    bad = np.nonzero((codes != want_c) | (roots != want_r).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} trees differ, the first at {bad[:8].tolist()}"


# -- a. more than one set-up block ------------------------------------------

@functools.lru_cache(maxsize=None)
def _block_case(W, T, name):
    cnt, leaves, blob = bg.block_batch(T, name)
    return cnt, leaves, blob, bg.model(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX)


@pytest.mark.parametrize("T", bg.BLOCK_T)
@pytest.mark.parametrize("W", [20, 32])
def test_blocks_of_trees_packed(engine, W, T):
    for name in bg.block_variants(T):
        cnt, leaves, blob, want = _block_case(W, T, name)
        assert ((want[1] != 0) == ((cnt == 0) | (cnt == 34))).all()
        same(engine.bmtree_roots(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX), want)


@pytest.mark.parametrize("T", bg.BLOCK_T)
@pytest.mark.parametrize("W", [20, 32])
def test_blocks_of_trees_dev(engine, W, T):
    for name in bg.block_variants(T):
        cnt, leaves, blob, want = _block_case(W, T, name)
        same(dev_roots(engine, W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX), want)


@pytest.mark.parametrize("counts", [[5] * 51 + [2] + [5] * 10, [5] * 50 + [9] + [5] * 10], ids=["2-leaf", "9-leaf"])
@pytest.mark.parametrize("W", [20, 32])
def test_bad_descriptor_in_a_tree_across_leaf_blocks(engine, W, counts):
    """leaves 255 and 256, the last lane of one block of the check and leaf
    kernels and the first of the next, are in one tree; a descriptor past the
    blob on its first leaf, on its last, and on both refuses it and leaves
    both neighbours exact"""
    cnt, leaves, blob = bg.sig_batch(counts, 31 + len(counts))
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    t = int(np.searchsorted(first, 255, side="right")) - 1
    lo, hi = first[t], first[t + 1] - 1
    assert lo <= 255 and hi >= 256 and t > 0 and t + 1 < len(cnt)
    for where in ([lo], [hi], [lo, hi]):
        lv = leaves.copy()
        lv["off"][where] = len(blob) - 63
        want = bg.model(W, cnt, lv, blob, 9)
        assert np.nonzero(want[1])[0].tolist() == [t]
        same(engine.bmtree_roots(W, cnt, lv, blob, 9), want)
        same(dev_roots(engine, W, cnt, lv, blob, 9), want)


@functools.lru_cache(maxsize=None)
def _bad_block_case(W):
    """600 trees: in the first block 100 trees of 17 and 33 leaves refused by
    one descriptor each (the first, a middle or the last leaf) between good
    ones, so that the check kernel's flags, and not the count rules, decide
    what the first block adds to the later blocks' offsets (1,300 nodes in
    layer 1 alone); the block tests above refuse by count only"""
    rng = np.random.default_rng(61 + W)
    counts = [(17, 33)[(t // 2) % 2] for t in range(200)] + rng.choice(bg.BLOCK_COUNTS, 400).tolist()
    cnt, leaves, blob = bg.sig_batch(counts, 62 + W)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    bad = list(range(0, 200, 2))
    for t in bad:
        k = (first[t], first[t] + counts[t] // 2, first[t + 1] - 1)[(t // 4) % 3]
        leaves["off"][k] = len(blob) - 63 + (t % 60)
    want = bg.model(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX)
    assert not want[1][1:200:2].any() and want[1][bad].all() and bg.layer_counts([counts[t] for t in bad], 33)[0] == 1300
    assert any(1 < c < 34 for c in counts[256:512]) and any(1 < c < 34 for c in counts[512:])
    return cnt, leaves, blob, want


@pytest.mark.parametrize("W", [20, 32])
def test_descriptor_refusals_ahead_of_later_blocks(engine, W):
    cnt, leaves, blob, want = _bad_block_case(W)
    same(engine.bmtree_roots(W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX), want)
    same(dev_roots(engine, W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX), want)


# -- b. more than one scan chunk ---------------------------------------------

SCAN_T = [262144, 262145, 524545]


@functools.lru_cache(maxsize=None)
def _scan_case(W, T):
    t = np.arange(T)
    counts = (7 * t + t // 256) % 6
    NB = (T + 255) // 256
    counts[(NB - 1) * 256:] = 5                      # the last block, and with it the only tree of a last chunk
    assert len(set(map(tuple, counts[:T // 256 * 256].reshape(-1, 256)[:6].tolist()))) == 6   # not periodic in 256
    cnt, leaves, blob = bg.pool_batch(counts, W, 900 + W)
    assert blob.nbytes == 4096 * W
    assert len(bg.layer_counts(counts[(NB - 1) * 256:], 5)) == 3
    want = bg.model(W, cnt, leaves, blob, 5, True)
    assert ((want[1] != 0) == (cnt == 0)).all()
    return cnt, leaves, blob, want


@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("W", [20, 32])
def test_scan_chunks_packed(engine, W, T):
    """NB = 1,024 block sums are one chunk of fd_k_bmtree_scan, 1,025 a second
    chunk of one block that holds one tree, 2,050 three chunks"""
    assert [(x + 255) // 256 for x in SCAN_T] == [1024, 1025, 2050]
    cnt, leaves, blob, want = _scan_case(W, T)
    same(engine.bmtree_roots(W, cnt, leaves, blob, 5, NODES), want)


@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("W", [20, 32])
def test_scan_chunks_dev(engine, W, T):
    cnt, leaves, blob, want = _scan_case(W, T)
    same(dev_roots(engine, W, cnt, leaves, blob, 5, NODES), want)


# -- c. lanes and capacities from the shapes alone -----------------------------

@pytest.mark.parametrize("nodes", [False, True], ids=["leaves", "nodes"])
@pytest.mark.parametrize("W", [20, 32])
def test_dev_lanes_and_capacities_met_exactly(engine, W, nodes):
    """one device call per shape: the lane bound of fd_bmtree_layer_bound is
    met with equality, node_b is filled to one below its capacity, and
    leaf_max is below N or far above it"""
    for shape, l in bg.TIGHT_LAYER.items():
        assert bg.layer_counts(shape, 1 << 30)[l - 1] == bg.layer_bound(len(shape), sum(shape), l)
    assert bg.layer_counts([3] * 300, 3)[0] == 600 == 2 * 900 // 3
    for k, counts in enumerate(bg.TIGHT_SHAPES):
        cnt, leaves, blob = bg.tight_batch(counts, W, nodes, 600 + k)
        for leaf_max in (max(counts), 1 << 30):
            assert leaf_max < len(leaves) or len(counts) == 1 or leaf_max == 1 << 30
            want = bg.model(W, cnt, leaves, blob, leaf_max, nodes)
            assert (want[1] == 0).all()
            same(dev_roots(engine, W, cnt, leaves, blob, leaf_max, NODES if nodes else 0), want)


# -- d. the leaf kernel --------------------------------------------------------

@pytest.mark.parametrize("W", [20, 32])
def test_one_odd_leaf_in_a_wave_of_signatures(engine, W):
    """64-byte leaves but one of 63 or 65 bytes: the odd leaf's wave takes the
    general body, every other wave the two-block one.  The odd leaf at lane
    0, 63, 64 (the first of the second wave), 129 (with 128 in the partial
    last wave) and 128 of 129 (alone in it); starts 4-byte aligned and odd;
    two-leaf trees, so the merge reads every node"""
    rng = np.random.default_rng(800 + W)
    for total, at in ((130, 0), (130, 63), (130, 64), (130, 129), (129, 128)):
        for odd in (63, 65):
            for name, align in (("aligned", lambda k: 4 * k), ("odd", lambda k: 2 * k + 1)):
                datas = [rng.bytes(odd if k == at else 64) for k in range(total)]
                trees = [datas[k:k + 2] for k in range(0, total, 2)]
                cnt, leaves, blob = bg.pack(trees, align_of=align)
                assert (leaves["sz"] != 64).sum() == 1 and leaves["sz"][at] == odd
                assert ((leaves["off"] % 4 == 0).all() if name == "aligned" else (leaves["off"] % 2 == 1).all())
                want = bg.model(W, cnt, leaves, blob, 2)
                assert (want[1] == 0).all()
                same(engine.bmtree_roots(W, cnt, leaves, blob, 2), want)


@pytest.mark.parametrize("W", [20, 32])
def test_largest_leaves(engine, W):
    """65,535 bytes (the largest accepted leaf; with the prefix byte a
    multiple of 64), 65,534, 65,527 and 65,526 (the last size whose padding
    fits its final block, and the first that needs one more) and 65,471, in
    one call of one-leaf and three-leaf trees; the last leaf ends the blob"""
    sizes = [65535, 65534, 65527, 65526, 65471]
    rng = np.random.default_rng(850 + W)
    trees = [[rng.bytes(s)] for s in sizes] + [[rng.bytes(s), rng.bytes(sizes[(i + 1) % 5]), rng.bytes(s)] for i, s in enumerate(sizes)]
    cnt, leaves, blob = bg.pack(trees, align_of=lambda k: 3 * k + 1)
    assert int(leaves[-1]["sz"]) == 65471 and int(leaves[-1]["off"]) + 65471 == len(blob)
    assert leaves["sz"].max() == fa.BMTREE_LEAF_SZ_MAX
    want = bg.model(W, cnt, leaves, blob, 3)
    assert (want[1] == 0).all()
    same(engine.bmtree_roots(W, cnt, leaves, blob, 3), want)
    same(dev_roots(engine, W, cnt, leaves, blob, 3), want)
