"""Merkle inclusion proof cases shared by the host, the sanitizer and the
device tests: the model (hashlib.sha256 layers, the proofs read off them, the
walk and the refusal rules, independent of the library) and the builders that
pack leaves, proofs and expected roots into one blob with its descriptors.
Not a test module."""
import hashlib

import numpy as np

import bmtree_grid as bg
import firedancer_amd as fa

EXPECT = fa.BMTREE_PROOF_EXPECT
FILL = 0xA5                     # the sentinel of proof rows


def ceil_log2(c: int) -> int:
    return (c - 1).bit_length() if c > 1 else 0


def merge(a: bytes, b: bytes, W: int) -> bytes:
    return hashlib.sha256(b"\x01" + a[:W] + b[:W]).digest()[:W]


def layers(nodes, W: int):
    """[layer 0 (the nodes), layer 1, .., [root]]"""
    out = [[bytes(x)[:W] for x in nodes]]
    assert out[0]
    while len(out[-1]) > 1:
        cur = out[-1]
        out.append([merge(cur[i], cur[i + 1] if i + 1 < len(cur) else cur[i], W) for i in range(0, len(cur), 2)])
    return out


def proofs(nodes, W: int):
    """the proof of every leaf: node l is layer l's (i >> l) ^ 1, or
    i >> l where the layer ends before it"""
    ls = layers(nodes, W)
    out = []
    for i in range(len(ls[0])):
        p = b""
        for l in range(len(ls) - 1):
            j = i >> l
            p += ls[l][j ^ 1 if (j ^ 1) < len(ls[l]) else j]
        out.append(p)
    return out


def walk(node: bytes, idx: int, proof: bytes, W: int, cnt: int = 0) -> bytes:
    """the derived root; cnt != 0: the strict walk of a tree of cnt leaves"""
    node = bytes(node)[:W]
    assert len(proof) % W == 0
    for l in range(len(proof) // W):
        p = proof[l * W:(l + 1) * W]
        if cnt and ((idx >> l) ^ 1) >= (cnt + (1 << l) - 1) >> l:
            node = merge(node, node, W)
        elif (idx >> l) & 1:
            node = merge(p, node, W)
        else:
            node = merge(node, p, W)
    return node


def refused(d, blob_sz: int, depth_max: int, W: int, nodes: bool) -> bool:
    """the header's refusal rules for one descriptor"""
    lim = min(blob_sz, 0xFFFFFFFF)
    leaf_off, leaf_sz, proof_off, idx, cnt, depth, expect_off, flags = (int(d[k]) for k in fa.BMTREE_PROOF_DTYPE.names)
    if flags & ~EXPECT or depth > depth_max:
        return True
    if leaf_off + leaf_sz > lim or leaf_sz > fa.BMTREE_LEAF_SZ_MAX or (nodes and leaf_sz != W):
        return True
    if proof_off + depth * W > lim or (flags & EXPECT and expect_off + W > lim):
        return True
    if cnt == 0:
        return depth < 32 and (idx >> depth) != 0
    return idx >= cnt or depth != ceil_log2(cnt)


def walk_model(W: int, desc, blob, depth_max: int, nodes: bool = False):
    """(roots (n, 32), codes) of a from-proofs call by the model"""
    raw = np.ascontiguousarray(blob, np.uint8).tobytes()
    roots = np.zeros((len(desc), 32), np.uint8)
    codes = np.zeros(len(desc), np.int32)
    for i, d in enumerate(desc):
        if refused(d, len(raw), depth_max, W, nodes):
            codes[i] = fa.ERR_ARG
            continue
        lo, sz, po, depth = int(d["leaf_off"]), int(d["leaf_sz"]), int(d["proof_off"]), int(d["depth"])
        node = raw[lo:lo + W] if nodes else bg.leaf(raw[lo:lo + sz], W)
        r = walk(node, int(d["idx"]), raw[po:po + depth * W], W, int(d["leaf_cnt"]))
        roots[i, :W] = np.frombuffer(r, np.uint8)
        if int(d["flags"]) & EXPECT and raw[int(d["expect_off"]):int(d["expect_off"]) + W] != r:
            codes[i] = fa.BMTREE_ERR_PROOF
    return roots, codes


def emit_model(W: int, leaf_cnt, leaves, blob, leaf_max: int, nodes: bool, stride: int):
    """(roots, codes, rows (n_leaves, stride)) of an emit call by the model:
    rows keep FILL wherever the call must not write"""
    roots, codes = bg.model(W, leaf_cnt, leaves, blob, leaf_max, nodes)
    raw = np.ascontiguousarray(blob, np.uint8).tobytes()
    leaves = np.asarray(leaves)
    rows = np.full((len(leaves), stride), FILL, np.uint8)
    at = 0
    for t, c in enumerate(np.asarray(leaf_cnt).tolist()):
        lo, at = at, at + c
        if codes[t]:
            continue
        off, sz = leaves["off"][lo:at].tolist(), leaves["sz"][lo:at].tolist()
        nd = [raw[o:o + W] if nodes else bg.leaf(raw[o:o + s], W) for o, s in zip(off, sz)]
        ls = layers(nd, W)
        assert ls[-1][0] == roots[t, :W].tobytes()
        for k, p in enumerate(proofs(nd, W)):
            assert len(p) == W * ceil_log2(c)
            rows[lo + k, :len(p)] = np.frombuffer(p, np.uint8)
    return roots, codes, rows


def stride_of(W: int, leaf_cnt, leaf_max: int) -> int:
    """the rows of the emit tests: W L and 12 bytes that no proof reaches"""
    return W * ceil_log2(min(leaf_max, int(np.asarray(leaf_cnt).sum()))) + 12


# -- from-proofs cases -------------------------------------------------------

class Blob:
    """pieces appended to one blob; put(data, at) starts the piece at an
    address that is `at` mod 16"""

    def __init__(self):
        self.buf = bytearray()

    def put(self, data: bytes, at=None) -> int:
        if at is not None:
            while len(self.buf) % 16 != at % 16:
                self.buf.append(0xEE)
        off = len(self.buf)
        self.buf += bytes(data)
        return off

    def array(self):
        return np.frombuffer(bytes(self.buf), np.uint8).copy()


def _desc(**k):
    d = np.zeros(1, fa.BMTREE_PROOF_DTYPE)[0]
    for name, v in k.items():
        d[name] = v
    return d


REFUSALS = ["leaf_past", "leaf_wraps", "proof_past", "proof_wraps", "expect_past", "expect_wraps", "leaf_sz", "depth_max",
            "flag_2", "flag_high", "idx_past_depth", "idx_past_cnt", "depth_short", "depth_long"]
SIZES = [0, 1, 54, 55, 56, 63, 64, 65, 119, 120, 128, 1139]


def walk_cases(W: int, nodes: bool = False):
    """The from-proofs grid as one call of mixed depths: (desc, blob,
    depth_max = 32, tags).  tags[i] names descriptor i's case and, where the
    case fixes it, its code; everything else comes from walk_model.  Proofs
    start at every address mod 16; the last proof ends the blob."""
    rng = np.random.default_rng(900 + W + nodes)
    b = Blob()
    desc, tags = [], []
    k = [0]

    def leaf_piece(sz=64):
        data = rng.bytes(W if nodes else sz)
        return data, (data if nodes else bg.leaf(data, W))

    def add(tag, data, proof, idx, cnt, expect=None, code=None, flags=None):
        lo = b.put(data)
        po = b.put(proof, at=k[0])
        k[0] += 1
        eo = b.put(expect) if expect is not None else 0
        fl = flags if flags is not None else (EXPECT if expect is not None else 0)
        desc.append(_desc(leaf_off=lo, leaf_sz=len(data), proof_off=po, idx=idx, leaf_cnt=cnt, depth=len(proof) // W,
                          expect_off=eo, flags=fl))
        tags.append((tag, code))

    # depth 0: the root is the leaf node
    for cnt in (0, 1):
        data, node = leaf_piece()
        add("depth0", data, b"", 0, cnt, expect=node, code=0)
    # depths 1..32 over random proof nodes: plain at a random index, strict at a random and at the last leaf
    for depth in range(1, 33):
        for kind in ("plain", "strict", "strict_last"):
            data, node = leaf_piece()
            proof = rng.bytes(depth * W)
            if kind == "plain":
                idx, cnt = (0xFFFFFFFF if depth == 32 else int(rng.integers(1 << depth))), 0
            else:
                cnt = 0xFFFFFFFF if depth == 32 else int(rng.integers((1 << (depth - 1)) + 1, (1 << depth) + 1))
                idx = cnt - 1 if kind == "strict_last" else int(rng.integers(cnt))
            add(f"depth{depth}_{kind}", data, proof, idx, cnt, expect=walk(node, idx, proof, W, cnt), code=0)
    # leaf sizes around the padding edges, each in a five-leaf tree
    if not nodes:
        for i, sz in enumerate(SIZES):
            datas = [rng.bytes(sz) for _ in range(5)]
            nd = [bg.leaf(d, W) for d in datas]
            add(f"size{sz}", datas[i % 5], proofs(nd, W)[i % 5], i % 5, 5 * (i & 1), expect=bg.root_of_nodes(nd, W), code=0)
    # an eleven-leaf tree: a flipped bit at each level of leaf 3's proof, and
    # leaf 10, whose level-0 node a strict walk never reads
    datas = [leaf_piece() for _ in range(11)]
    nd = [n for _, n in datas]
    root, pf = bg.root_of_nodes(nd, W), proofs(nd, W)
    for l in range(4):
        bad = bytearray(pf[3])
        bad[l * W + int(rng.integers(W))] ^= 1 << int(rng.integers(8))
        for cnt in (0, 11):
            add(f"flip{l}", datas[3][0], bytes(bad), 3, cnt, expect=root, code=fa.BMTREE_ERR_PROOF)
    bad = bytearray(pf[10])
    bad[int(rng.integers(W))] ^= 1 << int(rng.integers(8))
    add("unread_plain", datas[10][0], bytes(bad), 10, 0, expect=root, code=fa.BMTREE_ERR_PROOF)
    add("unread_strict", datas[10][0], bytes(bad), 10, 11, expect=root, code=0)
    add("no_expect", datas[10][0], bytes(bad), 10, 0, code=0)
    # room for a leaf above the size limit, so that only the size rule refuses it; then the proof that ends the blob
    b.put(b"\xEE" * (fa.BMTREE_LEAF_SZ_MAX + 2))
    add("last", datas[5][0], pf[5], 5, 11, code=0)
    desc[-1]["expect_off"] = len(b.buf)                   # past the blob, and not read without EXPECT
    blob = b.array()
    assert int(desc[-1]["proof_off"]) + 4 * W == len(blob)
    assert sorted({int(d["proof_off"]) % 16 for d in desc}) == list(range(16))
    # every refusal, one at a time: a valid descriptor with one field changed, each between valid ones
    base = next(d for d, (t, _) in zip(desc, tags) if t == "flip0" and d["leaf_cnt"] == 0).copy()
    base["flags"] = EXPECT
    eo = b.buf.find(root)
    base["expect_off"] = eo if eo >= 0 else 0
    n = len(blob)
    edits = {"leaf_past": dict(leaf_off=n - int(base["leaf_sz"]) + 1), "leaf_wraps": dict(leaf_off=0xFFFFFFF0),
             "proof_past": dict(proof_off=n - 4 * W + 1), "proof_wraps": dict(proof_off=0xFFFFFFF0),
             "expect_past": dict(expect_off=n - W + 1), "expect_wraps": dict(expect_off=0xFFFFFFF8),
             "leaf_sz": dict(leaf_off=0, leaf_sz=fa.BMTREE_LEAF_SZ_MAX + 1), "depth_max": dict(depth=33, proof_off=0),
             "flag_2": dict(flags=2 | EXPECT), "flag_high": dict(flags=0x80000000),
             "idx_past_depth": dict(idx=16), "idx_past_cnt": dict(leaf_cnt=11, idx=11),
             "depth_short": dict(leaf_cnt=17), "depth_long": dict(leaf_cnt=8, idx=3)}
    assert sorted(edits) == sorted(REFUSALS)
    for j, name in enumerate(REFUSALS):
        d = base.copy()
        for f, v in edits[name].items():
            d[f] = v
        at = 3 + 7 * j
        desc.insert(at, d)
        tags.insert(at, ("refuse_" + name, fa.ERR_ARG))
    return np.array(desc, fa.BMTREE_PROOF_DTYPE), blob, 32, tags


def check_walk_cases(desc, blob, depth_max, tags, W, nodes, roots, codes):
    """a from-proofs result against the model and against what the cases fix"""
    want_r, want_c = walk_model(W, desc, blob, depth_max, nodes)
    for i, (tag, code) in enumerate(tags):
        assert code is None or want_c[i] == code, (tag, int(want_c[i]))          # the model agrees with the case
        assert codes[i] == want_c[i], (tag, int(codes[i]), int(want_c[i]))
        assert (roots[i] == want_r[i]).all(), tag
        if code == fa.ERR_ARG:
            assert not roots[i].any(), tag
        elif tag.startswith("flip"):
            assert roots[i, :W].any()                                            # the derived root is still written
    assert (codes == fa.ERR_ARG).sum() == len(REFUSALS)
    if W == 20:
        assert not roots[:, 20:].any()


def tree_walk_batch(W: int, counts, nodes: bool, seed: int, strict: bool = True):
    """every leaf of every tree of a sig_batch / pool_batch with its model
    proof and its tree's root as EXPECT: (desc, blob, depth_max)"""
    cnt, leaves, blob = bg.tight_batch(counts, W, nodes, seed)
    raw = blob.tobytes()
    b = Blob()
    b.put(raw)
    desc = []
    at = 0
    for c in cnt.tolist():
        lo, at = at, at + c
        nd = [raw[int(o):int(o) + W] if nodes else bg.leaf(raw[int(o):int(o) + int(s)], W)
              for o, s in zip(leaves["off"][lo:at], leaves["sz"][lo:at])]
        eo = b.put(bg.root_of_nodes(nd, W))
        for k, p in enumerate(proofs(nd, W)):
            desc.append(_desc(leaf_off=leaves["off"][lo + k], leaf_sz=leaves["sz"][lo + k], proof_off=b.put(p), idx=k,
                              leaf_cnt=c if strict else 0, depth=ceil_log2(c), expect_off=eo, flags=EXPECT))
    return np.array(desc, fa.BMTREE_PROOF_DTYPE), b.array(), max(1, ceil_log2(max(cnt.tolist())))


# -- emit cases ----------------------------------------------------------------

EMIT_COUNTS = list(range(1, 71)) + [127, 128, 129, 255, 257]


def emit_grid(W: int, nodes: bool = False):
    """every count of EMIT_COUNTS once, shuffled: (leaf_cnt, leaves, blob, leaf_max)"""
    order = np.random.default_rng(500 + W).permutation(len(EMIT_COUNTS))
    counts = [EMIT_COUNTS[i] for i in order]
    return (*bg.tight_batch(counts, W, nodes, 600 + W), 257)
