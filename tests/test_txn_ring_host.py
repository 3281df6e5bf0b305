"""The claimed-slot rule of the ring's transaction batches
(include/fd_ed25519_gpu_txn.h, fd_ed25519_gpu_txn_claims): pure host code,
held against a statement of the rule in Python, entry by entry, and run as
a stand-alone program (tests/txn_ring_harness.cpp, its own main) under
AddressSanitizer and UndefinedBehaviorSanitizer over the same cases.  For
every entry, the reference parser accepting the payload implies that its
signature count is the claim: that is what lets the host lay out a ring
batch's slots before the device has parsed anything.  Nothing is loaded
into Python under a sanitizer.  Every comparison is exact."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import GOLDEN, ROOT
from firedancer_amd import corpus, txn

SRC = os.path.join(ROOT, "tests", "txn_ring_harness.cpp")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
MTU = corpus.TXN_MTU


def fixtures():
    return [open(os.path.join(GOLDEN, f"transaction{i}.bin"), "rb").read() for i in (1, 2, 3)]


def claim_rule(blob, off, sz):
    """the rule as the header states it"""
    if off + sz > len(blob) or sz < 1:
        return 0
    c = int(blob[off])
    return c if 1 <= c <= 127 else 0


def rule(blob, txns):
    claims = np.array([claim_rule(blob, int(o), int(s)) for o, s in zip(txns["off"], txns["sz"])], np.int64)
    bases = np.concatenate([[0], np.cumsum(claims)])
    return bases.astype(np.uint32), int(bases[-1])


def edge_case():
    """in bounds with first byte 0, 1, 127, 128, 255; sz == 0; off + sz == blob_sz and
    blob_sz + 1; off = 0xffffffff"""
    blob = np.zeros(64, np.uint8)
    blob[[0, 8, 16, 24, 32, 40, 63]] = [0, 1, 127, 128, 255, 9, 3]
    t = np.array([(0, 8), (8, 8), (16, 8), (24, 8), (32, 8), (40, 0), (40, 24), (40, 25), (63, 1), (63, 2), (64, 0), (64, 1),
                  (0xFFFFFFFF, 1), (0xFFFFFFFF, 0), (0xFFFFFFFF, 0xFFFFFFFF), (8, 1)], fa.TXN_DTYPE)
    return blob, t


def golden_case():
    return txn.pack(fixtures(), gap=3, first=1, pad=0)


def random_case(n=10000):
    """real transactions of 1..12 signatures, the fixtures and random bytes in one blob;
    entries on payload starts with their true sizes, random in-bounds windows, windows
    ending at and just past the blob's end, and offsets far outside"""
    rng = np.random.default_rng(31)
    b = corpus.solana_txns(300, seed=8, sig_dist=[1 / 12] * 12, max_sigs_per_txn=12)
    nreal = (len(b.blob) - 64) // MTU
    real = [bytes(b.blob[i * MTU:(i + 1) * MTU]) for i in range(nreal)] + fixtures()
    pb, pt = txn.pack(real, gap=1, first=2, pad=0)
    blob = np.concatenate([pb, rng.integers(0, 256, 4096, dtype=np.uint8)])
    n_b = len(blob)
    t = np.zeros(n, fa.TXN_DTYPE)
    kind = rng.integers(0, 8, n)
    for i in range(n):
        k = kind[i]
        if k < 3:
            t[i] = pt[int(rng.integers(0, len(pt)))]
        elif k < 5:
            off = int(rng.integers(0, n_b))
            t[i] = (off, int(rng.integers(0, n_b - off + 1)))
        elif k == 5:
            sz = int(rng.integers(0, 2000))
            t[i] = (n_b - sz + int(rng.integers(0, 2)), sz)          # ends at the end, or one byte past it
        elif k == 6:
            t[i] = (int(rng.integers(n_b, 1 << 32)), int(rng.integers(0, 1 << 32)))
        else:
            off = int(rng.integers(len(pb), n_b))                    # the random bytes: any first byte
            t[i] = (off, int(rng.integers(0, min(n_b - off, 300) + 1)))
    return blob, t


@pytest.fixture(scope="module")
def cases():
    return [edge_case(), golden_case(), random_case(), (np.zeros(0, np.uint8), np.array([(0, 0), (0, 1)], fa.TXN_DTYPE)),
            (np.array([5], np.uint8), np.zeros(0, fa.TXN_DTYPE))]


def test_edge_entries_by_hand():
    blob, t = edge_case()
    bases, n_sig = fa.txn_claims(blob, t)
    claims = np.diff(bases.astype(np.int64)).tolist()
    assert claims == [0, 1, 127, 0, 0, 0, 9, 0, 3, 0, 0, 0, 0, 0, 0, 1]
    assert n_sig == 141 and bases[0] == 0 and bases[-1] == 141


def test_claims_match_the_rule(cases):
    for blob, t in cases:
        bases, n_sig = fa.txn_claims(blob, t)
        want, total = rule(blob, t)
        assert bases.dtype == np.uint32 and len(bases) == len(t) + 1
        assert n_sig == total and np.array_equal(bases, want)
        # the total alone (bases == NULL)
        assert fa.lib().fd_ed25519_gpu_txn_claims(blob.ctypes.data if len(blob) else None, len(blob), t.ctypes.data if len(t) else None,
                                                  len(t), None) == total
    rb, rt = cases[2]
    claims = np.diff(fa.txn_claims(rb, rt)[0].astype(np.int64))
    assert len(rt) == 10000 and (claims > 0).sum() > 3000 and (claims == 0).sum() > 3000


def test_golden_transactions_claim_their_signature_counts():
    blob, t = golden_case()
    bases, n_sig = fa.txn_claims(blob, t)
    cnt = [txn.parse(p)["signature_cnt"] for p in fixtures()]
    assert np.diff(bases.astype(np.int64)).tolist() == cnt and n_sig == sum(cnt)


def test_a_parsed_payload_has_the_count_it_claims(cases, ref):
    """ref_txn_parse accepting the payload implies sig_cnt == claim, for every entry"""
    f = ref.ref_txn_parse
    f.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_ulong
    out = ctypes.create_string_buffer(1 << 19)
    parsed = 0
    for blob, t in cases:
        bases = fa.txn_claims(blob, t)[0].astype(np.int64)
        for i in range(len(t)):
            off, sz = int(t[i]["off"]), int(t[i]["sz"])
            if off + sz > len(blob):
                assert bases[i + 1] == bases[i]
                continue
            fp = f(blob.ctypes.data + off, sz, out, None)
            if fp:
                parsed += 1
                assert struct.unpack_from("<BB", out.raw, 0)[1] == bases[i + 1] - bases[i], (i, off, sz)
    assert parsed > 3000


def test_claims_under_asan_ubsan(cases, tmp_path):
    """the stand-alone program over the same cases: clean under both sanitizers, and the
    bases it writes are the rule's"""
    exe = tmp_path / "txn_ring_san"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *INC, "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)], check=True, capture_output=True)
    inp, outp = tmp_path / "cases.bin", tmp_path / "bases.bin"
    with open(inp, "wb") as fh:
        for blob, t in cases:
            fh.write(struct.pack("<QQ", len(blob), len(t)) + blob.tobytes() + t.tobytes())
    r = subprocess.run([str(exe), str(inp), str(outp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{len(cases)} cases, {sum(len(t) for _, t in cases)} entries ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    raw = open(outp, "rb").read()
    at = 0
    for blob, t in cases:
        want, total = rule(blob, t)
        assert struct.unpack_from("<Q", raw, at)[0] == total
        got = np.frombuffer(raw, np.uint32, len(t) + 1, at + 8)
        assert np.array_equal(got, want)
        at += 8 + 4 * (len(t) + 1)
    assert at == len(raw)
