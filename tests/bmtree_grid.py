"""Merkle tree test cases shared by the host and the device tests: the model
(hashlib.sha256, layer by layer, independent of the library), the golden
vectors and the batch builders.  Not a test module."""
import hashlib
import json
import os

import numpy as np

import firedancer_amd as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def leaf(data: bytes, W: int) -> bytes:
    return hashlib.sha256(b"\x00" + bytes(data)).digest()[:W]


def root_of_nodes(nodes, W: int) -> bytes:
    """the root over ready W-byte nodes: a layer of c > 1 nodes has
    ceil(c/2) parents, a node without a right sibling is merged with itself,
    a layer of one node is the root"""
    layer = [bytes(x)[:W] for x in nodes]
    assert layer
    while len(layer) > 1:
        if len(layer) & 1:
            layer.append(layer[-1])
        layer = [hashlib.sha256(b"\x01" + layer[i] + layer[i + 1]).digest()[:W] for i in range(0, len(layer), 2)]
    return layer[0]


def root(datas, W: int) -> bytes:
    return root_of_nodes([leaf(d, W) for d in datas], W)


def vectors():
    return json.load(open(os.path.join(GOLDEN, "bmtree_vectors.json")))


def v20_nodes(count: int) -> np.ndarray:
    """the reference's bmtree20 test leaves: node i = le64(i) || 0^12, as a (count, 20) byte array"""
    a = np.zeros((count, 20), np.uint8)
    a[:, :8] = np.arange(count, dtype="<u8").view(np.uint8).reshape(count, 8)
    return a


def refused(cnt: int, lf, blob_sz: int, leaf_max: int, W: int, nodes: bool) -> bool:
    """the header's refusal rules for one tree, lf its descriptors"""
    if cnt == 0 or cnt > leaf_max:
        return True
    for off, sz in lf:
        if int(off) + int(sz) > blob_sz or int(off) + int(sz) > 0xFFFFFFFF or sz > fa.BMTREE_LEAF_SZ_MAX or (nodes and sz != W):
            return True
    return False


def model(W: int, leaf_cnt, leaves, blob, leaf_max: int, nodes: bool = False):
    """(roots (n, 32), codes) of a batch by the model, refusals included: one
    pass over plain Python lists, so that half a million small trees take
    seconds"""
    raw = np.ascontiguousarray(blob, np.uint8).tobytes()
    leaves = np.asarray(leaves)
    off, sz = leaves["off"].tolist(), leaves["sz"].tolist()
    cnt = np.asarray(leaf_cnt).tolist()
    sha = hashlib.sha256
    out = bytearray(32 * len(cnt))
    codes = [0] * len(cnt)
    # the leaves that refuse their tree (refused() per leaf)
    end = leaves["off"].astype(np.uint64) + leaves["sz"]
    bad = (end > min(len(raw), 0xFFFFFFFF)) | (leaves["sz"] > fa.BMTREE_LEAF_SZ_MAX)
    if nodes:
        bad |= leaves["sz"] != W
    bad = bad.tolist() if bad.any() else None
    at = 0
    for t, c in enumerate(cnt):
        lo, at = at, at + c
        if c == 0 or c > leaf_max or (bad and True in bad[lo:at]):
            codes[t] = fa.ERR_ARG
            continue
        if nodes:
            layer = [raw[off[k]:off[k] + W] for k in range(lo, at)]
        else:
            layer = [sha(b"\x00" + raw[off[k]:off[k] + sz[k]]).digest()[:W] for k in range(lo, at)]
        while len(layer) > 1:
            if len(layer) & 1:
                layer.append(layer[-1])
            layer = [sha(b"\x01" + layer[i] + layer[i + 1]).digest()[:W] for i in range(0, len(layer), 2)]
        out[32 * t:32 * t + W] = layer[0]
    assert at == len(off)
    return np.frombuffer(bytes(out), np.uint8).reshape(len(cnt), 32).copy(), np.array(codes, np.int32)


def pack(datas_per_tree, align_of=None, tail_pad: int = 0):
    """trees of byte strings -> (leaf_cnt, leaves, blob).  align_of(k) gives
    the start alignment mod 16 of the k-th leaf (default: packed); tail_pad
    bytes follow the last leaf."""
    cnt = np.array([len(t) for t in datas_per_tree], np.uint32)
    total = int(cnt.sum())
    leaves = np.zeros(total, fa.BMTREE_LEAF_DTYPE)
    buf = bytearray()
    k = 0
    for t in datas_per_tree:
        for d in t:
            if align_of is not None:
                while len(buf) % 16 != align_of(k) % 16:
                    buf.append(0xEE)
            leaves[k] = (len(buf), len(d))
            buf += bytes(d)
            k += 1
    buf += b"\xEE" * tail_pad
    return cnt, leaves, np.frombuffer(bytes(buf), np.uint8).copy()


def sig_batch(counts, seed: int):
    """trees of random 64-byte leaves with the given counts, packed back to
    back: (leaf_cnt, leaves, blob)"""
    rng = np.random.default_rng(seed)
    cnt = np.array(counts, np.uint32)
    total = int(cnt.sum())
    blob = rng.integers(0, 256, 64 * total, dtype=np.uint8)
    leaves = np.zeros(total, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = np.arange(total, dtype=np.uint32) * 64
    leaves["sz"] = 64
    return cnt, leaves, blob


def refusal_batch(W: int, nodes: bool):
    """valid trees with one of every refusal between them: (leaf_cnt, leaves,
    blob, leaf_max, the refused trees' indices)"""
    rng = np.random.default_rng(40 + W + nodes)
    sz = W if nodes else 64
    trees = [[rng.bytes(sz) for _ in range(c)] for c in (3, 1, 5, 2, 4, 9, 3, 1, 6, 2, 7, 3, 2)]
    cnt, leaves, blob = pack(trees)
    if not nodes:   # room for a leaf of 65,536 bytes, so that only the size rule refuses it
        blob = np.concatenate([blob, np.full(fa.BMTREE_LEAF_SZ_MAX + 1 - len(blob), 0xEE, np.uint8)])
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
    leaves[first[3] + 1]["off"] = len(blob) - sz + 1      # tree 3: a leaf ends one byte past the blob
    leaves[first[7]]["off"] = 0xFFFFFFF0                  # tree 7: off + sz wraps 32 bits
    leaves[first[9]] = (0, fa.BMTREE_LEAF_SZ_MAX + 1)     # tree 9: a leaf above the size limit (node mode: sz != width)
    bad = [1, 3, 5, 7, 9]                                 # tree 5: 9 leaves > leaf_max 8
    if nodes:
        leaves[first[11] + 2]["sz"] = W - 1               # tree 11: sz != width
        bad.append(11)
    leaves = np.delete(leaves, first[1])                  # tree 1: no leaves
    cnt[1] = 0
    return cnt, leaves, blob, 8, bad


POOL = 4096


def pool_batch(counts, W: int, seed: int):
    """a node-mode batch (BMTREE_LEAVES_ARE_NODES) whose descriptors point at
    random into a shared pool of 4,096 random W-byte nodes: the blob stays
    small however many trees there are, and a tree that reads a neighbour's
    nodes does not land on equal data.  (leaf_cnt, leaves, blob)"""
    rng = np.random.default_rng(seed)
    cnt = np.array(counts, np.uint32)
    total = int(cnt.sum(dtype=np.uint64))
    blob = rng.integers(0, 256, POOL * W, dtype=np.uint8)
    leaves = np.zeros(total, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = W * rng.integers(0, POOL, total)
    leaves["sz"] = W
    return cnt, leaves, blob


def layer_counts(counts, leaf_max: int):
    """[nodes in layer 1, layer 2, ...] over the trees the count rules keep,
    down to the last layer that has any.  For choosing inputs and asserting
    that a chosen shape is what it is meant to be, never an expected result."""
    cs = [int(c) if 0 < int(c) <= leaf_max else 0 for c in counts]
    out = []
    while True:
        cs = [(c + 1) >> 1 if c > 1 else 0 for c in cs]
        if not any(cs):
            return out
        out.append(sum(cs))


def layer_bound(T: int, N: int, l: int) -> int:
    """fd_bmtree_layer_bound restated: the lanes a device call launches for layer l >= 1"""
    return (N >> l) + min(N // ((1 << (l - 1)) + 1), T)


# -- set-up blocks of 256 trees (FD_BMTREE_TB) ------------------------------

TB = 256
BLOCK_T = [255, 256, 257, 511, 512, 513, 1279]
BLOCK_COUNTS = [0, 1, 2, 3, 4, 5, 8, 9, 17, 33, 34]
BLOCK_LEAF_MAX = 33          # 34 is refused; 33 is the only count of depth 6


def _contributes(c) -> bool:
    return 1 < c <= BLOCK_LEAF_MAX


def block_variants(T: int):
    """{name: counts} of T trees with counts from BLOCK_COUNTS, placed around
    the blocks of 256 trees of the set-up kernels.  No batch can have a block
    that adds nothing between two that do, depth-6 trees on both sides of a
    block boundary and a refused and an empty tree on both sides of the same
    boundary all at once (257, 511 and 512 trees have one boundary), so each
    T runs as several calls and every property is asserted on the call built
    for it:
      mixed  any counts (every T)
      last   the only depth-6 tree of the call is its last tree (every T)
      deep   trees 255 and 256 are both of depth 6 (T > 256)
      edge   tree 255 is refused and tree 256 is empty (T > 256)
      dead   block 1 holds only empty, one-leaf and refused trees, tree 255
             refused and tree 256 empty, and blocks 0 and 2 contribute
             (T > 512: 513 and 1,279)"""
    rng = np.random.default_rng(7000 + T)
    draw = lambda: rng.choice(BLOCK_COUNTS, T).tolist()   # noqa: E731
    out = {"mixed": draw()}
    last = [c if c != 33 else 17 for c in draw()]
    last[T - 1] = 33
    out["last"] = last
    if T > TB:
        deep = draw()
        deep[TB - 1] = deep[TB] = 33
        out["deep"] = deep
        edge = draw()
        edge[TB - 1], edge[TB] = 34, 0
        out["edge"] = edge
    if T > 2 * TB:
        dead = draw()
        dead[TB:2 * TB] = rng.choice([0, 1, 34], TB).tolist()
        dead[TB - 1], dead[TB] = 34, 0
        dead[0], dead[2 * TB] = 9, 5
        out["dead"] = dead
    # the placement, asserted
    assert all(len(v) == T and set(v) <= set(BLOCK_COUNTS) for v in out.values())
    assert [i for i, c in enumerate(out["last"]) if c == 33] == [T - 1]
    assert len(layer_counts(out["last"], BLOCK_LEAF_MAX)) == 6 and layer_counts(out["last"], BLOCK_LEAF_MAX)[5] == 1
    if T > TB:
        assert out["deep"][TB - 1] == 33 and out["deep"][TB] == 33
        assert out["edge"][TB - 1] == 34 and out["edge"][TB] == 0
    if T > 2 * TB:
        d = out["dead"]
        assert not any(_contributes(c) for c in d[TB:2 * TB]) and {0, 1, 34} <= set(d[TB:2 * TB])
        assert any(_contributes(c) for c in d[:TB]) and any(_contributes(c) for c in d[2 * TB:])
        assert d[TB - 1] == 34 and d[TB] == 0
    return out


def block_batch(T: int, name: str):
    """variant `name` of block_variants(T) as 64-byte leaves: (leaf_cnt, leaves, blob)"""
    return sig_batch(block_variants(T)[name], 7100 + T)


# -- shapes that meet the device call's lane bound and capacities ------------

TIGHT_LAYER = {(3,): 1, (5, 5, 5): 2, (9, 9, 9): 3, (17, 1, 1): 5, (33, 1, 1): 6}   # shape: the layer it meets layer_bound in
TIGHT_SHAPES = [list(s) for s in TIGHT_LAYER] + [[3] * 300, [2, 1] * 200, [4097] + [1] * 300]


def tight_batch(counts, W: int, nodes: bool, seed: int):
    """one shape of TIGHT_SHAPES in node mode or as 64-byte leaves"""
    return pool_batch(counts, W, seed) if nodes else sig_batch(counts, seed)
