"""Merkle inclusion proofs on the host (fd_bmtree_proofs_batch and
fd_bmtree_from_proofs_batch): every proof byte, untouched byte, derived root
and code against the model of tests/bmtree_proof_grid.py, and every emitted
proof walked to the root the commit interface and the reference's vectors
give."""
import numpy as np
import pytest

import bmtree_grid as bg
import bmtree_proof_grid as pg
import firedancer_amd as fa

NODES = fa.BMTREE_LEAVES_ARE_NODES


def _rows(n, stride):
    return np.full((n, stride), pg.FILL, np.uint8)


@pytest.mark.parametrize("threads", [1, 5])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_every_count_in_one_shuffled_call(W, threads):
    cnt, leaves, blob, leaf_max = pg.emit_grid(W)
    stride = pg.stride_of(W, cnt, leaf_max)
    assert stride == W * 9 + 12
    want_r, want_c, want_p = pg.emit_model(W, cnt, leaves, blob, leaf_max, False, stride)
    roots, codes, rows = fa.bmtree_proofs_batch(W, cnt, leaves, blob, leaf_max, nthreads=threads, proofs=_rows(len(leaves), stride))
    assert (codes == 0).all() and (want_c == 0).all()
    assert (roots == want_r).all()
    assert (rows == want_p).all()                         # the proofs, and the sentinel past W D in every row
    assert (rows[:, W * 9:] == pg.FILL).all()
    r2, c2 = fa.bmtree_roots_batch(W, cnt, leaves, blob, leaf_max)
    assert (r2 == roots).all() and (c2 == codes).all()


@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_refused_trees_keep_their_rows(W, nodes):
    cnt, leaves, blob, leaf_max, bad = bg.refusal_batch(W, nodes)
    stride = pg.stride_of(W, cnt, leaf_max)
    want_r, want_c, want_p = pg.emit_model(W, cnt, leaves, blob, leaf_max, nodes, stride)
    assert sorted(np.nonzero(want_c)[0].tolist()) == bad
    roots, codes, rows = fa.bmtree_proofs_batch(W, cnt, leaves, blob, leaf_max, NODES if nodes else 0,
                                                proofs=_rows(len(leaves), stride))
    assert (codes == want_c).all() and (roots == want_r).all()
    assert (rows == want_p).all()
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    for t in bad:
        assert (rows[first[t]:first[t + 1]] == pg.FILL).all()


@pytest.mark.parametrize("W", [20, 32])
def test_every_emitted_proof_walks_to_the_commit_root(W):
    cnt, leaves, blob, leaf_max = pg.emit_grid(W)
    roots, codes, rows = fa.bmtree_proofs_batch(W, cnt, leaves, blob, leaf_max)
    raw = blob.tobytes()
    at = 0
    for t, c in enumerate(cnt.tolist()):
        lo, at = at, at + c
        nd = [bg.leaf(raw[int(o):int(o) + 64], W) for o in leaves["off"][lo:at]]
        root = fa.BmtreeCommit(W).append(nd).fini()
        assert root == roots[t, :W].tobytes()
        D = pg.ceil_log2(c)
        for k in range(c):
            p = rows[lo + k, :W * D].tobytes()
            assert pg.walk(nd[k], k, p, W) == root, (c, k)
            assert pg.walk(nd[k], k, p, W, c) == root, (c, k)


def _million(c, want):
    """the reference's million-leaf tree: the rows are emitted into the blob
    that the host walk then reads, every leaf strict with EXPECT at the
    recorded root (hashlib would take a minute for 20 million merges: it
    walks a sample)"""
    D = pg.ceil_log2(c)
    stride = 20 * D
    full = np.empty(20 * c + stride * c + 20, np.uint8)
    full[:20 * c] = bg.v20_nodes(c).reshape(-1)
    full[20 * c + stride * c:] = np.frombuffer(bytes.fromhex(want), np.uint8)
    rows = full[20 * c:20 * c + stride * c].reshape(c, stride)
    lv = np.zeros(c, fa.BMTREE_LEAF_DTYPE)
    lv["off"] = np.arange(c, dtype=np.uint32) * 20
    lv["sz"] = 20
    roots, codes, _ = fa.bmtree_proofs_batch(20, [c], lv, full[:20 * c], c, NODES, proofs=rows)
    assert codes[0] == 0 and roots[0, :20].tobytes().hex() == want
    desc = np.zeros(c, fa.BMTREE_PROOF_DTYPE)
    desc["leaf_off"] = lv["off"]
    desc["leaf_sz"] = 20
    desc["proof_off"] = 20 * c + stride * np.arange(c, dtype=np.uint32)
    desc["idx"] = np.arange(c, dtype=np.uint32)
    desc["leaf_cnt"] = c
    desc["depth"] = D
    desc["expect_off"] = 20 * c + stride * c
    desc["flags"] = pg.EXPECT
    got, codes = fa.bmtree_from_proofs_batch(20, desc, full, D, NODES, nthreads=8)
    assert (codes == 0).all()
    assert (got[:, :20] == np.frombuffer(bytes.fromhex(want), np.uint8)).all()
    for k in [0, 1, c - 1, c - 2, 524287, 524288] + np.random.default_rng(3).integers(0, c, 26).tolist():
        assert pg.walk(full[20 * k:20 * k + 20].tobytes(), k, rows[k].tobytes(), 20, c).hex() == want, k


def test_golden_node_mode_trees_walk_to_the_recorded_roots():
    v = bg.vectors()
    for c, want in v["bmtree20"]["roots"].items():
        c = int(c)
        if c > 4096:
            _million(c, want)
            continue
        nodes = bg.v20_nodes(c)
        lv = np.zeros(c, fa.BMTREE_LEAF_DTYPE)
        lv["off"] = np.arange(c, dtype=np.uint32) * 20
        lv["sz"] = 20
        roots, codes, rows = fa.bmtree_proofs_batch(20, [c], lv, nodes.reshape(-1), c, NODES)
        assert codes[0] == 0 and roots[0, :20].tobytes().hex() == want
        D = pg.ceil_log2(c)
        for k in range(c):
            assert pg.walk(nodes[k].tobytes(), k, rows[k, :20 * D].tobytes(), 20, c).hex() == want, (c, k)
    words = [w.encode() for w in v["bmtree32"]["leaves"]]
    nd = [bg.leaf(w, 32) for w in words]
    lv = np.zeros(11, fa.BMTREE_LEAF_DTYPE)
    lv["off"] = np.arange(11, dtype=np.uint32) * 32
    lv["sz"] = 32
    roots, codes, rows = fa.bmtree_proofs_batch(32, [11], lv, np.frombuffer(b"".join(nd), np.uint8), 11, NODES)
    assert codes[0] == 0 and roots[0].tobytes().hex() == v["bmtree32"]["root"]
    for k in range(11):
        assert pg.walk(nd[k], k, rows[k, :128].tobytes(), 32, 11).hex() == v["bmtree32"]["root"]


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_from_proofs_grid(W, nodes, threads):
    """depths 0..32, the leaf sizes, every refusal between valid descriptors,
    a flipped bit at each level and the node a strict walk never reads"""
    desc, blob, depth_max, tags = pg.walk_cases(W, nodes)
    names = {t for t, _ in tags}
    assert {"depth0", "depth32_plain", "depth32_strict", "unread_strict", "last"} <= names
    assert nodes or {f"size{s}" for s in pg.SIZES} <= names
    roots, codes = fa.bmtree_from_proofs_batch(W, desc, blob, depth_max, NODES if nodes else 0, nthreads=threads)
    pg.check_walk_cases(desc, blob, depth_max, tags, W, nodes, roots, codes)
    i32 = [i for i, (t, _) in enumerate(tags) if t == "depth32_plain"][0]
    assert desc[i32]["idx"] == 0xFFFFFFFF and desc[i32]["leaf_cnt"] == 0
    s32 = [i for i, (t, _) in enumerate(tags) if t == "depth32_strict"][0]
    assert desc[s32]["leaf_cnt"] == 0xFFFFFFFF
    # depth 0: the root is the leaf node
    i0 = [i for i, (t, _) in enumerate(tags) if t == "depth0"][0]
    lo, sz = int(desc[i0]["leaf_off"]), int(desc[i0]["leaf_sz"])
    node = blob[lo:lo + W].tobytes() if nodes else bg.leaf(blob[lo:lo + sz].tobytes(), W)
    assert roots[i0, :W].tobytes() == node
    # the strict walk does not read the flipped node; the plain walk does
    by = {t: i for i, (t, _) in enumerate(tags)}
    assert codes[by["unread_strict"]] == 0 and codes[by["unread_plain"]] == fa.BMTREE_ERR_PROOF


def test_from_proofs_depth_max_bounds_the_walk():
    desc, blob, depth_max = pg.tree_walk_batch(20, [3, 9, 5], False, 31)
    roots, codes = fa.bmtree_from_proofs_batch(20, desc, blob, 4)
    assert (codes == 0).all()
    roots, codes = fa.bmtree_from_proofs_batch(20, desc, blob, 3)
    want = np.where(desc["depth"] > 3, fa.ERR_ARG, 0)
    assert (codes == want).all() and want.any()
    assert not roots[want != 0].any()


@pytest.mark.parametrize("W", [20, 32])
def test_emit_then_from_proofs_round_trip(W):
    """the host emit's rows as the proofs of the host walk, in place"""
    cnt, leaves, blob = bg.sig_batch([1, 2, 3, 7, 8, 9, 33], 77)
    roots, codes, rows = fa.bmtree_proofs_batch(W, cnt, leaves, blob, 33)
    stride = rows.shape[1]
    base = len(blob)
    full = np.concatenate([blob, rows.reshape(-1), roots.reshape(-1)])
    desc = np.zeros(len(leaves), fa.BMTREE_PROOF_DTYPE)
    at = 0
    for t, c in enumerate(cnt.tolist()):
        for k in range(c):
            desc[at] = (leaves[at]["off"], 64, base + at * stride, k, c, pg.ceil_log2(c), base + rows.size + 32 * t, pg.EXPECT)
            at += 1
    got, codes = fa.bmtree_from_proofs_batch(W, desc, full, 6)
    assert (codes == 0).all()
    assert (got == np.repeat(roots, cnt, axis=0)).all()
