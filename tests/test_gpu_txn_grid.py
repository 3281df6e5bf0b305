"""The transaction grammar grid (tests/txn_grid.py; its own conditions are
checked on the CPU by tests/test_txn_grid.py) on the device: fd_k_txn_parse,
fd_k_txn_expand, fd_k_txn_reduce through Engine.verify_txns, debug_txn_descs
and verify_txns_dev, fd_k_txn_ring_front and fd_k_txn_ring_reduce through
submit_txns / poll_txns.

Expected values are those of tests/test_gpu_txn.py's `expect` and
tests/test_gpu_txn_ring.py's `ring_expect` / `check`, used as they are: the
reference build that travels with the tree says which payloads parse, gives the
descriptor, the footprint, the rejection's line and each signature's code.
Every comparison is exact."""
import re

import numpy as np
import pytest

import firedancer_amd as fa
import txn_grid as tg
from firedancer_amd import txn
from test_gpu_txn import FILL, DevCall, expect, same
from test_gpu_txn_ring import MAX_SIGS, check, claims_of, ring  # noqa: F401  (ring: a fixture)

pytestmark = pytest.mark.gpu

ORDERS = ("shuffled", "sorted")
# 22 is no footprint (20 + 10 instr_cnt + 8 tables): behind 20 comes 28
STRIDES = {20: 28, 256: 258, 3570: 3572, 4096: 4098}


class Run:
    """one order of the grid, packed at odd offsets with gaps, and what the reference says"""


@pytest.fixture(scope="module")
def runs(ref):
    g = tg.grid()
    out = {}
    for name in ORDERS:
        r = Run()
        r.cases = [g.cases[i] for i in getattr(g, name)]
        r.blob, r.t = txn.pack([c.payload for c in r.cases], gap=3, first=1)
        assert (r.t["off"] & 1).any() and not (r.t["off"] & 1).all()
        r.exp, r.codes, r.descs, r.raws = expect(ref, r.blob, r.t)
        r.fp = np.array([len(x) for x in r.raws])
        out[name] = r
    return out


def named(cases, fn, *args):
    """fn(*args) (same, or check: used as they are), a failure naming the first differing case"""
    try:
        return fn(*args)
    except AssertionError as e:
        why = str(e).splitlines()[0] if str(e) else "differs"
        at = re.search(r"first at (\d+)", why)
        raise AssertionError(f"{why} -- {cases[int(at.group(1))]!r}" if at else why) from None


def first_diff(cases, got, exp):
    """'' if equal, else the case of the first differing row"""
    bad = np.nonzero(got != exp)[0]
    return repr(cases[int(bad[0])]) if len(bad) else ""


def rows_of(raws, stride):
    want = np.zeros((len(raws), stride), np.uint8)
    for t, raw in enumerate(raws):
        if 0 < len(raw) <= stride:
            want[t, :len(raw)] = np.frombuffer(raw, np.uint8)
    return want


@pytest.mark.parametrize("order", ORDERS)
def test_synchronous_path(engine, runs, order):
    """a. verify_txns on the whole grid: every result field, every code"""
    r = runs[order]
    got, codes, _ = engine.verify_txns(r.blob, r.t, want_codes=True)
    named(r.cases, same, got, r.exp)
    assert np.array_equal(codes, r.codes)
    st = r.exp["status"]
    assert (st == 0).sum() > 1000 and (st == fa.ERR_TXN).sum() > 700 and (st == fa.ERR_SIG).sum() >= 10 and (st == fa.ERR_MSG).sum() >= 10
    assert set(r.exp["reject_line"][st == fa.ERR_TXN].tolist()) == set(tg.LINES)
    assert (r.fp > 65535).sum() >= 10 and (r.exp["footprint"][r.fp > 65535] == 65535).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_descriptors_at_stride(engine, runs, order, stride):
    """b. a row holds exactly the reference's descriptor where 0 < footprint <= stride and
    is zero otherwise: footprint == stride is written, the next footprint is not, and the
    giants' rows stay zero while their footprint field saturates"""
    r = runs[order]
    got, codes, out = engine.verify_txns(r.blob, r.t, want_codes=True, txn_out_stride=stride)
    named(r.cases, same, got, r.exp)
    assert np.array_equal(codes, r.codes)
    assert not first_diff(r.cases, out, rows_of(r.raws, stride))
    at, past = np.nonzero(r.fp == stride)[0], np.nonzero(r.fp == STRIDES[stride])[0]
    assert len(at) and len(past)
    assert all(out[i].tobytes() == r.raws[i] for i in at) and not out[past].any()
    big = r.fp > 65535
    assert big.sum() >= 10 and not out[big].any() and (got["footprint"][big] == 65535).all()


@pytest.mark.parametrize("order", ORDERS)
def test_expansion_alone(engine, runs, order):
    """c. debug_txn_descs: the reference-derived descriptors one after another, the fill
    descriptors behind them, sig_base the prefix sum of the counts"""
    r = runs[order]
    n = len(r.descs)
    desc, n_sig, res = engine.debug_txn_descs(r.blob, r.t, n + 7)
    assert n_sig == n, first_diff(r.cases, res["sig_cnt"], r.exp["sig_cnt"])
    assert np.array_equal(desc[:n], r.descs)
    assert desc[n:].tolist() == [FILL] * 7
    cnt = r.exp["sig_cnt"].astype(np.int64)
    assert np.array_equal(res["sig_base"], np.cumsum(cnt) - cnt)
    e = r.exp.copy()
    e["status"][e["status"] != fa.ERR_TXN] = 0          # nothing was verified: no signature's code yet
    named(r.cases, same, res, e)


def test_lone_launches(engine, ref, runs):
    """d. n_txn == 1: every giant, the footprint-20 payload, one payload of every reject line"""
    r = runs["sorted"]
    pick = set(np.nonzero(np.array([len(c.payload) for c in r.cases]) > tg.GIANT)[0].tolist())
    pick.add(int(np.nonzero(r.fp == 20)[0][0]))
    lines = r.exp["reject_line"]
    for line in tg.LINES:
        pick.add(int(np.nonzero(lines == line)[0][0]))          # the smallest payload of that line
    assert len(pick) >= 60
    for i in sorted(pick):
        blob, t = txn.pack([r.cases[i].payload], gap=3, first=1)
        exp, ecodes, _, raws = expect(ref, blob, t)
        got, codes, out = engine.verify_txns(blob, t, want_codes=True, txn_out_stride=256)
        named([r.cases[i]], same, got, exp)
        assert np.array_equal(codes, ecodes), r.cases[i]
        assert np.array_equal(out, rows_of(raws, 256)), r.cases[i]
        assert exp["footprint"][0] == min(r.fp[i], 65535) and exp["reject_line"][0] == lines[i]


def test_device_resident_path(engine, ref, runs):
    """e. verify_txns_dev on the shuffled grid with sig_cap at the total and at the
    sig_base of a giant: that giant and every parsed transaction behind it get ERR_ARG"""
    import torch
    r = runs["shuffled"]
    n, total = len(r.t), len(r.codes)
    sz = np.array([len(c.payload) for c in r.cases])
    giants = np.nonzero((sz > tg.GIANT) & (r.exp["sig_cnt"] > 0))[0]
    cut = int(giants[len(giants) // 2])
    assert 0 < r.exp["sig_base"][cut] < total
    exp = expect(ref, r.blob[:len(r.blob) - 64], r.t)
    same(exp[0], r.exp)
    for cap, first_out in ((total, n), (int(r.exp["sig_base"][cut]), cut)):
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        call = DevCall(r.blob, r.t, cap, stride=256)
        torch.cuda.synchronize()
        call.launch(engine, stream)
        stream.synchronize()
        got, codes, out = call.fetch()
        e = r.exp.copy()
        over = (np.arange(n) >= first_out) & (e["sig_cnt"] > 0)
        e["status"][over] = fa.ERR_ARG
        named(r.cases, same, got, e)
        assert np.array_equal(codes[:cap], r.codes[:cap])
        assert not first_diff(r.cases, out, rows_of(r.raws, 256))
        assert over.sum() == (0 if first_out == n else (r.exp["sig_cnt"][cut:] > 0).sum())


def test_ring(ring, ref, runs):  # noqa: F811
    """f. the shuffled grid through submit_txns / poll_txns in batches that fit the ring
    engine (at most 4,096 claimed signatures, its blob size); rejected payloads that claim
    slots keep them, with ERR_ARG codes"""
    r = runs["shuffled"]
    ps = list(r.cases)
    room = ring.max_blob - 64 - 1
    assert max(len(c.payload) for c in ps) + 3 <= room                # no payload needs an engine of its own
    batches, cur, claimed, used = [], [], 0, 0
    for c in ps:
        p = c.payload
        if cur and (claimed + tg.claims(p) > MAX_SIGS or used + len(p) + 3 > room or len(cur) == MAX_SIGS):
            batches.append(cur)
            cur, claimed, used = [], 0, 0
        cur.append(c)
        claimed += tg.claims(p)
        used += len(p) + 3
    batches.append(cur)
    assert sum(len(b) for b in batches) == len(ps) and len(batches) >= 3
    kept = 0
    for b in batches:
        blob, t = txn.pack([c.payload for c in b], gap=3, first=1)
        assert blob.nbytes <= ring.max_blob and int(claims_of(blob, t).sum()) <= MAX_SIGS
        got, codes = named(b, check, ring, ref, blob, t)
        claim = claims_of(blob, t)
        for i in np.nonzero((got["status"] == fa.ERR_TXN) & (claim > 0))[0]:
            lo = int(got["sig_base"][i])
            assert got["sig_cnt"][i] == 0 and (codes[lo:lo + claim[i]] == fa.ERR_ARG).all()
            assert i + 1 == len(b) or got["sig_base"][i + 1] == lo + claim[i]
            kept += 1
    assert kept >= 200
