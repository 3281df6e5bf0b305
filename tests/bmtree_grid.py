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
    """(roots (n, 32), codes) of a batch by the model, refusals included"""
    blob = np.ascontiguousarray(blob, np.uint8)
    raw = blob.tobytes()
    roots = np.zeros((len(leaf_cnt), 32), np.uint8)
    codes = np.zeros(len(leaf_cnt), np.int32)
    at = 0
    for t, c in enumerate(leaf_cnt):
        c = int(c)
        lf = [(int(d["off"]), int(d["sz"])) for d in leaves[at:at + c]]
        at += c
        if refused(c, lf, len(raw), leaf_max, W, nodes):
            codes[t] = fa.ERR_ARG
            continue
        parts = [raw[o:o + s] for o, s in lf]
        r = root_of_nodes(parts, W) if nodes else root(parts, W)
        roots[t, :W] = np.frombuffer(r, np.uint8)
    return roots, codes


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
