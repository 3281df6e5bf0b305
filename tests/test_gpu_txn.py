"""Whole transactions on the device (include/fd_ed25519_gpu_txn.h): parse,
scan, expand, the unchanged verify pipeline, reduce.

Expected values come from the reference build that travels with the tree:
ref_txn_parse says which payloads parse and gives the descriptor, the
footprint and the rejection's source line; ref_verify_batch
(oracle/_ref/libfdref.so, libfdref_portable.so for MODE_PORTABLE) gives each
signature's code, and the first nonzero one in signature order is the
transaction's status.  The expansion test alone follows the issue's own
wording and compares with txn.descs_for.  Every comparison is exact."""
import ctypes
import os
import struct

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import GOLDEN, P, ROOT
from firedancer_amd import corpus, txn

pytestmark = pytest.mark.gpu

MTU = corpus.TXN_MTU
FILL = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)        # the tail-slot descriptor
L_ORDER = (2**252 + 27742317777372353535851937790883648493).to_bytes(32, "little")


def fixtures():
    return [open(os.path.join(GOLDEN, f"transaction{i}.bin"), "rb").read() for i in (1, 2, 3)]


@pytest.fixture(scope="module")
def refp():
    path = os.path.join(ROOT, "oracle", "_ref", "libfdref_portable.so")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: build it with make -C oracle ref")
    return ctypes.CDLL(path)


def ref_codes(L, fn, b):
    sig, pub, data, off, sz = b.flat()
    out = np.zeros(len(b), np.int32)
    getattr(L, fn)(ctypes.c_uint64(len(b)), P(sig), P(pub), P(data), P(off), P(sz), P(out), min(16, os.cpu_count() or 8))
    return out


def expect(ref, blob, txns, portable=None):
    """What the reference says about a batch -> (results, codes, descs, raws):
    results as TXN_RESULT_DTYPE, codes per signature, descs the descriptors of
    every parsed transaction's signatures, raws[t] the fd_txn_t bytes (b'' if
    malformed).  An entry outside the blob is ERR_ARG and is not looked at.
    portable: the FD_HAS_AVX=0 build, whose codes replace the AVX build's."""
    f = ref.ref_txn_parse
    f.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_ulong
    n = len(txns)
    res = np.zeros(n, fa.TXN_RESULT_DTYPE)
    res["version"] = 0xFF
    out = ctypes.create_string_buffer(1 << 19)
    ctr = txn.Counters()
    base, raws, dl = blob.ctypes.data, [], []
    n_sig = 0
    for t in range(n):
        off, sz = int(txns[t]["off"]), int(txns[t]["sz"])
        res[t]["sig_base"] = n_sig
        if off + sz > len(blob):
            res[t]["status"] = fa.ERR_ARG
            raws.append(b"")
            continue
        ctr.failure_cnt = 0
        fp = f(base + off, sz, out, ctypes.byref(ctr))
        if not fp:
            res[t]["status"], res[t]["reject_line"] = fa.ERR_TXN, ctr.failure_ring[0]
            raws.append(b"")
            continue
        raw = out.raw[:fp]
        ver, k, so, mo = struct.unpack_from("<BBHH", raw, 0)
        ao, = struct.unpack_from("<H", raw, 10)
        res[t]["tag"] = int.from_bytes(bytes(blob[off + so:off + so + 8]), "little")
        res[t]["footprint"], res[t]["sig_cnt"], res[t]["version"] = min(fp, 0xFFFF), k, ver
        d = np.zeros(k, fa.DESC_DTYPE)
        j = np.arange(k)
        d["sig_off"], d["pub_off"], d["msg_off"], d["msg_sz"] = off + so + 64 * j, off + ao + 32 * j, off + mo, sz - mo
        dl.append(d)
        raws.append(raw)
        n_sig += k
    descs = np.concatenate(dl) if dl else np.zeros(0, fa.DESC_DTYPE)
    if not len(descs):
        codes = np.zeros(0, np.int32)
    elif portable is not None:
        codes = ref_codes(portable, "refp_verify_batch", corpus.Batch(blob, descs))
    else:
        codes = ref_codes(ref, "ref_verify_batch", corpus.Batch(blob, descs))
    # the first nonzero code of each parsed transaction's signatures
    nz = np.nonzero(codes)[0]
    lo = res["sig_base"].astype(np.int64)
    first = np.searchsorted(nz, lo)
    hit = (res["sig_cnt"] > 0) & (first < len(nz))
    hit[hit] = nz[first[hit]] < lo[hit] + res["sig_cnt"][hit]
    res["status"][hit] = codes[nz[first[hit]]]
    return res, codes, descs, raws


def same(got, exp):
    for f in ("status", "sig_base", "tag", "footprint", "reject_line", "sig_cnt", "version"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, f"{f}: {len(bad)} differ, first at {bad[0]}: got {got[f][bad[0]]}, expected {exp[f][bad[0]]}"
    assert not got["_pad"].any()


@pytest.fixture(scope="module")
def txns12():
    """4,200 transactions of 1..12 signatures (C2 shape, all valid)"""
    b = corpus.solana_txns(28500, seed=21, sig_dist=[1 / 12] * 12, max_sigs_per_txn=12)
    n = (len(b.blob) - 64) // MTU
    assert n >= 4200
    return [bytes(b.blob[t * MTU:(t + 1) * MTU]) for t in range(n)]


@pytest.fixture(scope="module")
def twelve():
    """transactions of exactly 12 signatures"""
    b = corpus.solana_txns(12 * 24, seed=22, sig_dist=[0] * 11 + [1], max_sigs_per_txn=12)
    return [bytes(b.blob[t * MTU:(t + 1) * MTU]) for t in range(24)]


def test_parser_on_device(engine, ref):
    """all truncations of the three fixtures and all 255 mutations of every byte of
    transaction2.bin (v0 with lookup tables): every result field, every descriptor at
    stride 256, and the status -- ERR_TXN where the reference returns 0, else the first
    nonzero reference code (most mutants parse and fail ERR_MSG / ERR_SIG / ERR_PUBKEY)"""
    fx = fixtures()
    p2 = np.frombuffer(fx[1], np.uint8)
    n2 = len(p2)
    mut = np.tile(p2, (255 * n2, 1))
    pos = np.repeat(np.arange(n2), 255)
    mut[np.arange(255 * n2), pos] = (p2[pos] + np.tile(np.arange(1, 256), n2)).astype(np.uint8)
    trunc = [p[:i] for p in fx for i in range(len(p) + 1)]
    tb, tt = txn.pack(trunc, gap=1, first=3, pad=0)
    blob = np.concatenate([tb, mut.reshape(-1), np.zeros(64, np.uint8)])
    txns = np.zeros(len(trunc) + len(mut), fa.TXN_DTYPE)
    txns[:len(trunc)] = tt
    txns["off"][len(trunc):] = len(tb) + n2 * np.arange(len(mut))
    txns["sz"][len(trunc):] = n2
    exp, ecodes, _, raws = expect(ref, blob, txns)
    got, codes, out = engine.verify_txns(blob, txns, want_codes=True, txn_out_stride=256)
    same(got, exp)
    assert np.array_equal(codes, ecodes)
    st = set(exp["status"].tolist())
    assert {fa.ERR_TXN, fa.ERR_MSG, 0} <= st and len(st & {fa.ERR_SIG, fa.ERR_PUBKEY}) >= 1
    want = np.zeros_like(out)
    for t, raw in enumerate(raws):
        if 0 < len(raw) <= 256:
            want[t, :len(raw)] = np.frombuffer(raw, np.uint8)
    assert np.array_equal(out, want)
    assert (exp["footprint"] > 0).sum() > 50000 and (exp["status"] == fa.ERR_TXN).sum() > 10000


def _spoil(payloads, where):
    out = list(payloads)
    for k, w in enumerate(where):
        if 0 <= w < len(out):
            out[w] = [out[w][:-1], b"\x00" + out[w][1:], out[w] + b"\x00", b""][k % 4]
    return out


@pytest.mark.parametrize("n_txn", [1, 63, 64, 65, 257, 4097])
def test_expansion(engine, txns12, n_txn):
    """debug_txn_descs == the concatenation of txn.descs_for, payloads at odd offsets with
    gaps, malformed ones first, last, at a wave edge and at a scan-block edge"""
    ps = txns12[:n_txn]
    if n_txn > 1:
        ps = _spoil(ps, [0, n_txn - 1, 63, 64, 255, 256, 1023, 1024])
    blob, t = txn.pack(ps, gap=3, first=1)
    assert (t["off"] & 1).any()
    dl = [txn.descs_for(p, int(o)) for p, o in zip(ps, t["off"])]
    want = np.concatenate([d for d in dl if d is not None])
    desc, n_sig, res = engine.debug_txn_descs(blob, t, len(want) + 5)
    assert n_sig == len(want)
    assert np.array_equal(desc[:n_sig], want)
    assert desc[n_sig:].tolist() == [FILL] * 5
    cnt = np.array([0 if d is None else len(d) for d in dl])
    assert np.array_equal(res["sig_cnt"], cnt)
    assert np.array_equal(res["sig_base"], np.cumsum(cnt) - cnt)
    assert np.array_equal(res["status"] == fa.ERR_TXN, cnt == 0)


def test_expansion_past_a_million_transactions(engine, txns12):
    """2^20 + 3 entries (the scan's single block walks 4,097 block sums in five rounds):
    entries may alias the same bytes, so 61 payloads stand for all of them"""
    ps = _spoil(txns12[:61], [5, 17, 18, 40])
    blob, t61 = txn.pack(ps, gap=1, first=1)
    n = (1 << 20) + 3
    pick = (np.arange(n) * 7) % 61
    pick[np.arange(n) % 32 != 0] = 18              # 31 in 32 are the empty payload: 2^18 slots suffice
    t = t61[pick]
    dl = [txn.descs_for(p, int(o)) for p, o in zip(ps, t61["off"])]
    cnt61 = np.array([0 if d is None else len(d) for d in dl])
    cnt = cnt61[pick]
    base = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    assert total + 2 <= engine.max_sigs and cnt61[18] == 0
    desc, n_sig, res = engine.debug_txn_descs(blob, t, total + 2)
    assert n_sig == total and desc[total:].tolist() == [FILL] * 2
    assert np.array_equal(res["sig_cnt"], cnt) and np.array_equal(res["sig_base"], base)
    want = np.concatenate([dl[k] for k in pick[cnt > 0]])
    assert np.array_equal(desc[:total], want)


def test_all_malformed_and_127_signatures(engine, ref):
    ps = [b"", b"\x00" * 40, b"\x05" + b"\x01" * 100, fixtures()[0][:-1], b"\x80"]
    blob, t = txn.pack(ps, gap=1, first=1)
    desc, n_sig, res = engine.debug_txn_descs(blob, t, 16)
    assert n_sig == 0 and desc.tolist() == [FILL] * 16
    exp = expect(ref, blob, t)[0]
    same(res, exp)
    got, codes, _ = engine.verify_txns(blob, t, want_codes=True)     # 9 signatures claimed, none real
    same(got, exp)
    assert (got["status"] == fa.ERR_TXN).all() and len(codes) == 0
    # one transaction of 127 signatures (far past the MTU): built here, signed by the host signer
    k = 127
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    pubs = fa.lib().fd_ed25519_public_batch
    pub = np.zeros((k, 32), np.uint8)
    pubs(k, P(seeds), P(pub), 4)
    msg = bytes([k, 0, 1, 0x80, 0x01]) + pub.tobytes() + bytes(rng.integers(0, 256, 32, dtype=np.uint8)) * 2 + bytes([1, k, 0, 0])
    body = np.frombuffer(msg, np.uint8).copy()
    _, sig = fa.sign_batch(seeds, body, np.zeros(k, np.uint64), np.full(k, len(msg), np.uint32))
    payload = bytes([k]) + sig.tobytes() + msg
    bad = bytearray(payload)
    bad[1 + 64 * 126 + 3] ^= 4                     # R of the last signature
    ps = [fixtures()[2], payload, bytes(bad), fixtures()[1]]
    blob, t = txn.pack(ps, gap=5, first=7)
    exp, ecodes, edesc, _ = expect(ref, blob, t)
    assert exp["sig_cnt"].tolist()[1:3] == [127, 127] and exp["status"][1] == 0 and exp["status"][2] != 0
    desc, n_sig, _ = engine.debug_txn_descs(blob, t, len(edesc))
    assert n_sig == len(edesc) and np.array_equal(desc, edesc)
    got, codes, _ = engine.verify_txns(blob, t, want_codes=True)
    same(got, exp)
    assert np.array_equal(codes, ecodes)


def test_first_failing_code_in_signature_order(engine, ref, twelve):
    """S of signature a set to L (ERR_SIG), a bit of R of signature b flipped: the
    transaction's status is the code of whichever comes first"""
    pos = [0, 1, 6, 11]
    ps, who = [twelve[0]], [None]
    i = 1
    for a in pos:
        for b in pos:
            if a == b:
                continue
            p = bytearray(twelve[i % len(twelve)])
            p[1 + 64 * a + 32:1 + 64 * a + 64] = L_ORDER
            p[1 + 64 * b + 2] ^= 0x10
            ps.append(bytes(p))
            who.append((a, b))
            i += 1
    last = bytearray(twelve[5])
    last[1 + 64 * 11 + 40] ^= 1                    # only the last signature is bad
    ps.append(bytes(last))
    who.append("last")
    blob, t = txn.pack(ps, gap=1, first=1)
    exp, ecodes, _, _ = expect(ref, blob, t)
    got, codes, _ = engine.verify_txns(blob, t, want_codes=True)
    same(got, exp)
    assert np.array_equal(codes, ecodes)
    assert exp["status"][0] == 0 and exp["status"][-1] != 0 and (ecodes[-12:-1] == 0).all()
    for w, s, base in zip(who, got["status"], got["sig_base"]):
        if isinstance(w, tuple):
            a, b = w
            assert ecodes[base + a] == fa.ERR_SIG and ecodes[base + b] not in (0, fa.ERR_SIG)
            assert s == (fa.ERR_SIG if a < b else ecodes[base + b])


def test_semantics_carried_through(engine, ref, refp, twelve, txns12):
    """a Q1 early-accept S, a small-order signer and a non-canonical signer inside
    transactions: the AVX build's codes, and the portable build's under MODE_PORTABLE"""
    ps = [txns12[0], txns12[1]]
    q1 = bytearray(twelve[1])
    q1[1 + 64 * 3 + 63] = 0x10                     # s[31] = 0x10: S >= L that the reference's AVX build accepts as a scalar
    ps.append(bytes(q1))
    for enc in corpus.small_order_encodings()[:6]:
        p = bytearray(twelve[2])
        ao = txn.parse(bytes(p))["acct_addr_off"]
        p[ao + 32 * 4:ao + 32 * 5] = enc           # signer 4
        ps.append(bytes(p))
    for enc in (b"\xff" * 31 + b"\x7f", b"\xee" + b"\xff" * 30 + b"\x7f", b"\xed" + b"\xff" * 30 + b"\xff"):
        p = bytearray(twelve[3])
        ao = txn.parse(bytes(p))["acct_addr_off"]
        p[ao:ao + 32] = enc                        # the fee payer, y >= p
        ps.append(bytes(p))
    ps.append(txns12[2])
    blob, t = txn.pack(ps, gap=2, first=5)
    exp_avx = expect(ref, blob, t)
    exp_port = expect(ref, blob, t, portable=refp)
    assert not np.array_equal(exp_avx[1], exp_port[1])      # the two builds do differ on this batch
    assert engine.mode == fa.MODE_AVX
    got, codes, _ = engine.verify_txns(blob, t, want_codes=True)
    same(got, exp_avx[0])
    assert np.array_equal(codes, exp_avx[1])
    engine.mode = fa.MODE_PORTABLE
    try:
        got, codes, _ = engine.verify_txns(blob, t, want_codes=True)
    finally:
        engine.mode = fa.MODE_AVX
    same(got, exp_port[0])
    assert np.array_equal(codes, exp_port[1])


def test_bounds(engine, ref, txns12):
    """entries past the blob, near 2^32, of size 0 and 65,536: the documented code, the
    neighbours unaffected"""
    good = txns12[:6]
    blob, t = txn.pack(good, gap=1, first=1, pad=0)
    blob = np.concatenate([blob, np.zeros(70000, np.uint8)])
    blob[len(blob) - 66000] = 1
    n = len(blob)
    extra = np.array([(n - 10, 11), (0xFFFFFFF0, 100), (0xFFFFFFFF, 0xFFFFFFFF), (n, 1), (n, 0), (5, 0), (n - 66000, 65536),
                      (n - 66000, 65535), (n - MTU + 1, MTU)], fa.TXN_DTYPE)
    order = [0, 6, 1, 7, 8, 2, 9, 10, 3, 11, 12, 4, 13, 14, 5]
    allt = np.concatenate([t, extra])[order]
    exp, ecodes, _, _ = expect(ref, blob, allt)
    assert exp["status"].tolist() == [0, fa.ERR_ARG, 0, fa.ERR_ARG, fa.ERR_ARG, 0, fa.ERR_ARG, fa.ERR_TXN, 0, fa.ERR_TXN,
                                      fa.ERR_TXN, 0, fa.ERR_TXN, fa.ERR_ARG, 0]
    assert exp["reject_line"].tolist() == [0, 0, 0, 0, 0, 0, 0, 79, 0, 79, 73, 0, exp["reject_line"][12], 0, 0]
    got, codes, _ = engine.verify_txns(blob, allt, want_codes=True)
    same(got, exp)
    assert np.array_equal(codes, ecodes)


class DevCall:
    """one verify_txns_dev call on torch tensors: upload at construction, launch(), fetch()"""

    def __init__(self, blob, txns, sig_cap, stride=0):
        import torch
        dev = torch.device("cuda", 0)
        self.n, self.cap, self.stride, self.blob_sz = len(txns), sig_cap, stride, len(blob) - 64   # txn.pack's pad
        self.d_blob = torch.from_numpy(blob).to(dev)
        self.d_txn = torch.from_numpy(txns.view(np.uint8).copy()).to(dev)
        self.d_res = torch.full((self.n * 3,), -1, dtype=torch.int64, device=dev)
        self.d_codes = torch.full((max(sig_cap, 1),), 77, dtype=torch.int32, device=dev)
        self.d_out = torch.zeros(max(self.n * stride, 2), dtype=torch.uint8, device=dev)

    def launch(self, engine, stream):
        engine.verify_txns_dev(self.n, self.d_blob.data_ptr(), self.blob_sz, self.d_txn.data_ptr(), self.cap, self.d_res.data_ptr(),
                               self.d_codes.data_ptr(), self.d_out.data_ptr() if self.stride else 0, self.stride, stream.cuda_stream)

    def fetch(self):
        return (self.d_res.cpu().numpy().view(fa.TXN_RESULT_DTYPE).copy(), self.d_codes.cpu().numpy()[:self.cap],
                self.d_out.cpu().numpy()[:self.n * self.stride].reshape(self.n, self.stride) if self.stride else None)


def test_sig_cap_one_below_total(engine, ref, txns12):
    """device path: exactly the transactions past sig_cap get ERR_ARG, the rest their codes"""
    import torch
    ps = _spoil(txns12[100:140], [3, 38])
    bad = bytearray(ps[10])
    bad[1 + 5] ^= 1
    ps[10] = bytes(bad)
    blob, t = txn.pack(ps, gap=1, first=1)
    exp, ecodes, _, _ = expect(ref, blob[:len(blob) - 64], t)
    total = len(ecodes)
    last = int(np.nonzero(exp["sig_cnt"])[0][-1])
    assert exp["sig_cnt"][20] > 0
    for cap, cut in ((total, len(ps)), (total - 1, last), (int(exp["sig_base"][20]), 20), (int(exp["sig_base"][25]) + 1, 25)):
        if cut == 25 and exp["sig_cnt"][25] < 2:
            continue
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        call = DevCall(blob, t, cap)
        torch.cuda.synchronize()
        call.launch(engine, stream)
        stream.synchronize()
        got, codes, _ = call.fetch()
        e = exp.copy()
        over = (np.arange(len(ps)) >= cut) & (e["sig_cnt"] > 0)
        e["status"][over] = fa.ERR_ARG
        same(got, e)
        fit = int(exp["sig_base"][cut]) if cut < len(ps) else total
        assert np.array_equal(codes[:fit], ecodes[:fit])
        assert (codes[fit:] == fa.ERR_ARG).all()           # tail slots


def test_packed_call_chunks_past_max_sigs(ref, txns12):
    """a packed call claiming more than the engine's max_sigs == the reference on the whole
    batch (a small engine: 256 signatures a launch)"""
    small = fa.Engine(0, 256, 1 << 21)
    try:
        ps = _spoil(txns12[200:460], [0, 77, 259])
        for w in (5, 130):
            p = bytearray(ps[w])
            p[1 + 33] ^= 2
            ps[w] = bytes(p)
        blob, t = txn.pack(ps, gap=0, first=0)
        exp, ecodes, _, raws = expect(ref, blob, t)
        assert len(ecodes) > 4 * 256
        small.txns_reserve(64)
        got, codes, out = small.verify_txns(blob, t, want_codes=True, txn_out_stride=32)
        same(got, exp)
        assert np.array_equal(codes, ecodes)
        for r, raw in zip(out, raws):
            assert bytes(r) == (raw + b"\0" * (32 - len(raw)) if 0 < len(raw) <= 32 else b"\0" * 32)
        parts = [small.verify_txns(blob, t[i:i + 20], want_codes=True) for i in range(0, len(t), 20)]
        assert np.array_equal(np.concatenate([p[0]["status"] for p in parts]), got["status"])
        assert np.array_equal(np.concatenate([p[1] for p in parts]), codes)
    finally:
        small.close()


def test_paths_agree_and_back_to_back(engine, ref, txns12):
    """packed == device-resident == verify_packed on host-made descriptors plus a host
    reduction; two device calls in a row on one stream, nothing between them"""
    import torch
    batches = []
    for lo, hi, sp in ((500, 900, [7, 100]), (900, 1500, [0, 599])):
        ps = _spoil(txns12[lo:hi], sp)
        for w in range(3, len(ps), 37):
            p = bytearray(ps[w])
            p[1 + 64 * (w % max(p[0], 1)) + 40] ^= 1
            ps[w] = bytes(p)
        batches.append(txn.pack(ps, gap=1, first=1))
    exps = [expect(ref, b[:len(b) - 64], t) for b, t in batches]
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    calls = [DevCall(b, t, len(e[1]) + 9, stride=64) for (b, t), e in zip(batches, exps)]
    torch.cuda.synchronize()
    for c in calls:
        c.launch(engine, stream)                    # back to back: nothing between the two
    stream.synchronize()
    for (b, t), e, c in zip(batches, exps, calls):
        res, codes, out = c.fetch()
        same(res, e[0])
        assert np.array_equal(codes[:len(e[1])], e[1]) and (codes[len(e[1]):] == fa.ERR_ARG).all()
        pres, pcodes, pout = engine.verify_txns(b[:len(b) - 64], t, want_codes=True, txn_out_stride=64)
        same(pres, res)
        assert np.array_equal(pcodes, e[1])
        for t_i, raw in enumerate(e[3]):
            if 0 < len(raw) <= 64:
                assert bytes(out[t_i][:len(raw)]) == raw and bytes(pout[t_i][:len(raw)]) == raw
        hc = engine.verify_packed(b, e[2])
        assert np.array_equal(hc, e[1])
        red = [next((int(c) for c in hc[s:s + k] if c), 0) for s, k in zip(res["sig_base"], res["sig_cnt"])]
        ok = res["sig_cnt"] > 0
        assert np.array_equal(np.array(red)[ok], res["status"][ok])
    assert engine.verify_txns(batches[0][0], batches[0][1]).dtype == fa.TXN_RESULT_DTYPE
