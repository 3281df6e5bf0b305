"""Merkle inclusion proofs on the device (fd_k_bmtree_proof_gather and
fd_k_bmtree_from_proof through Engine.bmtree_proofs, bmtree_proofs_dev,
bmtree_from_proofs and bmtree_from_proofs_dev): every proof byte, every
untouched byte, every derived root and every code against the model of
tests/bmtree_proof_grid.py (hashlib, layer by layer)."""
import functools

import numpy as np
import pytest

import bmtree_grid as bg
import bmtree_proof_grid as pg
import firedancer_amd as fa

pytestmark = pytest.mark.gpu

NODES = fa.BMTREE_LEAVES_ARE_NODES


def _emit_and_check(engine, W, cnt, leaves, blob, leaf_max, nodes):
    stride = pg.stride_of(W, cnt, leaf_max)
    want_r, want_c, want_p = pg.emit_model(W, cnt, leaves, blob, leaf_max, nodes, stride)
    flags = NODES if nodes else 0
    roots, codes, rows = engine.bmtree_proofs(W, cnt, leaves, blob, leaf_max, flags, proofs=np.full_like(want_p, pg.FILL))
    assert (codes == want_c).all()
    assert (roots == want_r).all()
    assert (rows == want_p).all()                         # the proofs, the sentinel past W D and in the rows of refused trees
    r2, c2 = engine.bmtree_roots(W, cnt, leaves, blob, leaf_max, flags)
    assert (r2 == roots).all() and (c2 == codes).all()
    return want_c


@functools.lru_cache(maxsize=None)
def _grid(W, nodes):
    cnt, leaves, blob, leaf_max = pg.emit_grid(W, nodes)
    stride = pg.stride_of(W, cnt, leaf_max)
    return cnt, leaves, blob, leaf_max, stride, pg.emit_model(W, cnt, leaves, blob, leaf_max, nodes, stride)


@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_every_count_in_one_shuffled_call(engine, W, nodes):
    cnt, leaves, blob, leaf_max, stride, (want_r, want_c, want_p) = _grid(W, nodes)
    assert (want_c == 0).all()
    flags = NODES if nodes else 0
    roots, codes, rows = engine.bmtree_proofs(W, cnt, leaves, blob, leaf_max, flags, proofs=np.full_like(want_p, pg.FILL))
    assert (codes == 0).all() and (roots == want_r).all()
    assert (rows == want_p).all()
    assert (rows[:, stride - 12:] == pg.FILL).all()
    r2, c2 = engine.bmtree_roots(W, cnt, leaves, blob, leaf_max, flags)
    assert (r2 == roots).all() and (c2 == codes).all()
    host_r, host_c, host_p = fa.bmtree_proofs_batch(W, cnt, leaves, blob, leaf_max, flags, proofs=np.full_like(want_p, pg.FILL))
    assert (host_r == roots).all() and (host_c == codes).all() and (host_p == rows).all()


@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_refused_trees_keep_their_rows(engine, W, nodes):
    cnt, leaves, blob, leaf_max, bad = bg.refusal_batch(W, nodes)
    want_c = _emit_and_check(engine, W, cnt, leaves, blob, leaf_max, nodes)
    assert sorted(np.nonzero(want_c)[0].tolist()) == bad


@pytest.mark.parametrize("shape", [[4097] + [1] * 300, [33, 1, 1], [17, 1, 1], [3] * 300], ids=["4097", "33", "17", "3x300"])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_where_a_layer_buffer_is_reused(engine, W, shape):
    """shapes that meet the lane bound and the capacities: a gather that ran
    after the merge launch that overwrites its layer, or read past a
    capacity, would show here"""
    assert shape in bg.TIGHT_SHAPES
    nodes = W == 32
    cnt, leaves, blob = bg.tight_batch(shape, W, nodes, 800 + len(shape))
    want_c = _emit_and_check(engine, W, cnt, leaves, blob, max(shape), nodes)
    assert (want_c == 0).all()


@pytest.mark.parametrize("T,name", [(257, "edge"), (513, "dead"), (1279, "mixed")])
@pytest.mark.parametrize("W", [20, 32])
def test_emit_across_the_set_up_blocks(engine, W, T, name):
    cnt, leaves, blob = bg.block_batch(T, name)
    want_c = _emit_and_check(engine, W, cnt, leaves, blob, bg.BLOCK_LEAF_MAX, False)
    assert (want_c != 0).any() and (want_c == 0).any()


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_dev_strided_rows_into_sentinels(engine, W, own_stream):
    import torch
    cnt, leaves, blob, leaf_max, stride, (want_r, want_c, want_p) = _grid(W, False)
    T, N = len(cnt), len(leaves)
    pitch, lead = 13 * W + 40, 28                         # the rows start 28 bytes into a pitch of their own; 12 levels fit (below)
    assert lead + stride <= pitch and pitch >= W * pg.ceil_log2(N)
    dev = torch.device("cuda", 0)
    first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_roots = torch.full((T, 112), 0x5A, dtype=torch.uint8, device=dev)
    d_rows = torch.full((N, pitch), pg.FILL, dtype=torch.uint8, device=dev)
    d_codes = torch.full((T,), 77, dtype=torch.int32, device=dev)
    d_work = torch.zeros(fa.bmtree_work_sz(T, N), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (W, T, d_first.data_ptr(), N, d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, leaf_max, d_roots.data_ptr() + 32, 112,
            d_rows.data_ptr() + lead, pitch, d_codes.data_ptr(), d_work.data_ptr())
    if own_stream:
        stream = torch.cuda.Stream(dev)
        engine.bmtree_proofs_dev(*args, stream.cuda_stream)
        stream.synchronize()
    else:
        engine.bmtree_proofs_dev(*args)
        torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    got = d_roots.cpu().numpy()
    assert (got[:, 32:64] == want_r).all()
    assert (got[:, :32] == 0x5A).all() and (got[:, 64:] == 0x5A).all()
    rows = d_rows.cpu().numpy()
    assert (rows[:, lead:lead + stride] == want_p).all()
    assert (rows[:, :lead] == pg.FILL).all() and (rows[:, lead + stride:] == pg.FILL).all()
    # leaf_max far past every tree: the extra gather and merge launches find nothing to do
    d_rows.fill_(pg.FILL)
    d_codes.fill_(77)
    torch.cuda.synchronize()
    engine.bmtree_proofs_dev(*args[:7], 1 << 30, *args[8:10], d_rows.data_ptr(), pitch, *args[12:])
    torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    rows = d_rows.cpu().numpy()
    assert (rows[:, :stride] == want_p).all() and (rows[:, stride:] == pg.FILL).all()


# -- from proofs ---------------------------------------------------------------

@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_from_proofs_grid_in_one_call(engine, W, nodes):
    """depths 0..32, the leaf sizes, every refusal, the flipped bits and the
    unread node in one call, proofs at every address mod 16: the lanes of a
    wave differ in depth, leaf size and path"""
    desc, blob, depth_max, tags = pg.walk_cases(W, nodes)
    assert sorted({int(d["proof_off"]) % 16 for d in desc}) == list(range(16))
    roots, codes = engine.bmtree_from_proofs(W, desc, blob, depth_max, NODES if nodes else 0)
    pg.check_walk_cases(desc, blob, depth_max, tags, W, nodes, roots, codes)
    host_r, host_c = fa.bmtree_from_proofs_batch(W, desc, blob, depth_max, NODES if nodes else 0)
    assert (host_r == roots).all() and (host_c == codes).all()


@functools.lru_cache(maxsize=None)
def _uniform(W, nodes):
    counts = [1, 2, 3, 5, 8, 13, 21, 34, 55, 70, 45]     # 257 leaves
    desc, blob, depth_max = pg.tree_walk_batch(W, counts, nodes, 950 + W, strict=not nodes)
    assert len(desc) == 257
    return desc, blob, depth_max, pg.walk_model(W, desc, blob, depth_max, nodes)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("W", [20, 32])
def test_from_proofs_wave_uniform_paths_and_lane_counts(engine, W, nodes, n):
    """64-byte leaves only (the two-block leaf body) and ready nodes, over
    one lane, a wave less one, a wave, a wave and one, and a block and one"""
    desc, blob, depth_max, (want_r, want_c) = _uniform(W, nodes)
    assert (want_c == 0).all() and (nodes or (desc["leaf_sz"] == 64).all())
    roots, codes = engine.bmtree_from_proofs(W, desc[:n], blob, depth_max, NODES if nodes else 0)
    assert (codes == 0).all()
    assert (roots == want_r[:n]).all()


def test_from_proofs_one_flipped_payload_bit(engine):
    desc, blob, depth_max, (want_r, _) = _uniform(20, False)
    flipped = blob.copy()
    k = 200
    flipped[int(desc[k]["leaf_off"]) + 17] ^= 0x10
    assert sum(1 for d in desc if d["leaf_off"] == desc[k]["leaf_off"]) == 1
    want_r, want_c = pg.walk_model(20, desc, flipped, depth_max)
    assert want_c[k] == fa.BMTREE_ERR_PROOF and (np.delete(want_c, k) == 0).all()
    roots, codes = engine.bmtree_from_proofs(20, desc, flipped, depth_max)
    assert (codes == want_c).all() and (roots == want_r).all()


def test_from_proofs_dev_strided_roots_and_empty_call(engine):
    import torch
    desc, blob, depth_max, (want_r, want_c) = _uniform(32, False)
    n = len(desc)
    dev = torch.device("cuda", 0)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_roots = torch.full((n, 80), 0x5A, dtype=torch.uint8, device=dev)
    d_codes = torch.full((n,), 77, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    engine.bmtree_from_proofs_dev(32, n, d_desc.data_ptr(), d_blob.data_ptr(), blob.nbytes, depth_max, d_roots.data_ptr() + 16, 80,
                                  d_codes.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = d_roots.cpu().numpy()
    assert (d_codes.cpu().numpy() == want_c).all()
    assert (got[:, 16:48] == want_r).all()
    assert (got[:, :16] == 0x5A).all() and (got[:, 48:] == 0x5A).all()
    roots, codes = engine.bmtree_from_proofs(32, desc[:0], blob, depth_max)
    assert len(roots) == 0 and len(codes) == 0


# -- shreds: emit into the tails, walk in place, verify the signed root ---------

ROW, PAYLOAD, TAIL = 1228, 64, 1108                      # a row: signature | payload (the leaf) | proof of depth 6
SETS = [33, 48, 64]


def test_shred_shaped_round_trip(engine):
    import torch
    rng = np.random.default_rng(1234)
    R = sum(SETS)
    first = np.concatenate([[0], np.cumsum(SETS)]).astype(np.uint32)
    set_of = np.repeat(np.arange(3), SETS)
    idx_in = np.arange(R) - first[set_of]
    pub_off, sroot_off = R * ROW, R * ROW + 96             # rows | 3 public keys | 3 set roots | R derived roots
    droot_off = sroot_off + 96
    total = droot_off + 32 * R
    host = np.zeros(total, np.uint8)
    host[:R * ROW] = rng.integers(0, 256, R * ROW, dtype=np.uint8)
    rows = host[:R * ROW].reshape(R, ROW)
    rows[:, TAIL:] = pg.FILL
    leaves = np.zeros(R, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = np.arange(R, dtype=np.uint32) * ROW + PAYLOAD
    leaves["sz"] = TAIL - PAYLOAD
    assert all(pg.ceil_log2(c) == 6 for c in SETS) and TAIL + 6 * 20 == ROW
    want_r, want_c, want_p = pg.emit_model(20, SETS, leaves, host, 64, False, 120)
    assert (want_c == 0).all()

    dev = torch.device("cuda", 0)
    d_blob = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    d_blob[:total] = torch.from_numpy(host).to(dev)
    d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
    d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
    d_tcodes = torch.full((3,), 77, dtype=torch.int32, device=dev)
    d_work = torch.zeros(fa.bmtree_work_sz(3, R), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)                       # one stream of the caller's orders the walk before the verify
    s = stream.cuda_stream
    assert s
    torch.cuda.synchronize()
    base = d_blob.data_ptr()
    # leader: the set roots into the blob, every proof into its row's tail
    engine.bmtree_proofs_dev(20, 3, d_first.data_ptr(), R, d_leaves.data_ptr(), base, R * ROW, 64, base + sroot_off, 32,
                             base + TAIL, ROW, d_tcodes.data_ptr(), d_work.data_ptr(), s)
    torch.cuda.synchronize()
    assert (d_tcodes.cpu().numpy() == 0).all()
    got = d_blob.cpu().numpy()[:total]
    assert (got[sroot_off:sroot_off + 96].reshape(3, 32) == want_r).all()
    assert (got[:R * ROW].reshape(R, ROW)[:, TAIL:] == want_p).all()
    assert (got[:R * ROW].reshape(R, ROW)[:, :TAIL] == rows[:, :TAIL]).all()

    # receiver: leaf and proof in place, strict, EXPECT at the set's root
    desc = np.zeros(R, fa.BMTREE_PROOF_DTYPE)
    desc["leaf_off"] = leaves["off"]
    desc["leaf_sz"] = leaves["sz"]
    desc["proof_off"] = np.arange(R, dtype=np.uint32) * ROW + TAIL
    desc["idx"] = idx_in
    desc["leaf_cnt"] = np.array(SETS)[set_of]
    desc["depth"] = 6
    desc["expect_off"] = sroot_off + 32 * set_of
    desc["flags"] = pg.EXPECT
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_scratch = torch.zeros((R, 32), dtype=torch.uint8, device=dev)
    d_codes = torch.full((R,), 77, dtype=torch.int32, device=dev)
    engine.bmtree_from_proofs_dev(20, R, d_desc.data_ptr(), base, total, 6, d_scratch.data_ptr(), 32, d_codes.data_ptr(), s)
    torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    assert (d_scratch.cpu().numpy() == want_r[set_of]).all()

    # one payload byte of one row flipped: that row alone misses its root
    victim = 33 + 17
    got[victim * ROW + PAYLOAD + 500] ^= 0x04
    # the leader's signatures over the 20-byte roots, one key per set, into row[0, 64) of every row
    seeds = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    pub, sig = fa.sign_batch(seeds, want_r.reshape(-1), np.arange(3, dtype=np.uint64) * 32, np.full(3, 20, np.uint32))
    got[pub_off:pub_off + 96] = pub.reshape(-1)
    got[:R * ROW].reshape(R, ROW)[:, :64] = sig[set_of]
    d_blob[:total] = torch.from_numpy(got.copy()).to(dev)
    d_codes.fill_(77)
    torch.cuda.synchronize()
    engine.bmtree_from_proofs_dev(20, R, d_desc.data_ptr(), base, total, 6, d_scratch.data_ptr(), 32, d_codes.data_ptr(), s)
    torch.cuda.synchronize()
    codes = d_codes.cpu().numpy()
    assert codes[victim] == fa.BMTREE_ERR_PROOF and (np.delete(codes, victim) == 0).all()

    # without EXPECT the derived roots go into the reserved tail of the blob and are the verify call's messages in place
    desc["flags"] = 0
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    vdesc = np.zeros(R, fa.DESC_DTYPE)
    vdesc["sig_off"] = np.arange(R, dtype=np.uint32) * ROW
    vdesc["pub_off"] = pub_off + 32 * set_of
    vdesc["msg_off"] = droot_off + 32 * np.arange(R, dtype=np.uint32)
    vdesc["msg_sz"] = 20
    d_vdesc = torch.from_numpy(vdesc.view(np.uint8).copy()).to(dev)
    d_out = torch.full((R,), 99, dtype=torch.int32, device=dev)
    d_codes.fill_(77)
    torch.cuda.synchronize()
    engine.bmtree_from_proofs_dev(20, R, d_desc.data_ptr(), base, droot_off, 6, base + droot_off, 32, d_codes.data_ptr(), s)
    engine.verify_dev(R, base, total, d_vdesc.data_ptr(), d_out.data_ptr(), s)
    torch.cuda.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    derived = d_blob.cpu().numpy()[droot_off:total].reshape(R, 32)
    model_r, _ = pg.walk_model(20, desc, got, 6)
    assert (derived == model_r).all()
    assert (np.delete(derived, victim, axis=0) == np.delete(want_r[set_of], victim, axis=0)).all()
    out = d_out.cpu().numpy()
    assert out[victim] == fa.ERR_MSG and (np.delete(out, victim) == 0).all()
