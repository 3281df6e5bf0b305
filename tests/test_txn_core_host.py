"""The parser core (firedancer_amd/csrc/fd_txn_core.h: what fd_k_txn_parse
runs one lane per transaction) compiled for the host by
tests/txn_core_harness.cpp and held against the library's fd_txn_parse, the
reference parser compiled in place (fixture ref) and the golden digests the
reference produced -- over the reference's own test_mutate sweep, random
payloads and a > 64 KiB payload.  Every comparison is exact.  The harness
parses each payload from the end of a heap block of exactly its size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from firedancer_amd import corpus, txn
from test_txn import _parser, fixtures, golden, sweep

SRC = os.path.join(ROOT, "tests", "txn_core_harness.cpp")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]


def build_harness(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *INC, *extra, SRC, "-o", str(out)], check=True, capture_output=True)


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    so = tmp_path_factory.mktemp("txn_core") / "txn_core_harness.so"
    build_harness(so, ("-O2", "-shared", "-fPIC"))
    L = ctypes.CDLL(str(so))
    vp, ul = ctypes.c_void_p, ctypes.c_ulong
    L.core_txn_cmp.argtypes = [ctypes.c_char_p, ul, vp]
    L.core_txn_cmp.restype = ctypes.c_int
    L.core_txn_sweep_cmp.argtypes = [ctypes.c_char_p, ul, vp, vp]
    L.core_txn_sweep_cmp.restype = ul
    L.core_txn_summary.argtypes = [ctypes.c_char_p, ul, vp]
    L.core_txn_summary.restype = ul
    return L


def _addr(L, name):
    return ctypes.cast(getattr(L, name), ctypes.c_void_p)


def test_core_compiles_as_c(tmp_path):
    """one source of truth: fd_txn_host.c includes the core, so it is C too"""
    src = tmp_path / "core.c"
    src.write_text('#include "fd_txn_core.h"\n'
                   "unsigned long f( uint8_t const * p, unsigned long n, fd_txn_core_sum_t * s ) { return fd_txn_core_parse( p, n, 0, 0UL, s ); }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", *INC, "-c", str(src), "-o", str(tmp_path / "core.o")],
                   check=True, capture_output=True)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_core_sweep_matches_golden(core, k):
    """digests of (footprint, descriptor bytes) and the counters, failure ring included"""
    digest, ctr = sweep(_parser(core, "core_txn_parse"), fixtures()[k])
    exp = golden()["sweep"][k]
    assert digest == exp["sha256"]
    assert ctr == (exp["success_cnt"], exp["failure_cnt"], exp["failure_ring"])


@pytest.mark.parametrize("k", [0, 1, 2])
def test_core_sweep_vs_library_and_reference(core, ref, k):
    """per payload: footprint, descriptor bytes, reject_line against failure_ring[0] of a
    fresh counter, sig_cnt, version, acct_addr_off and tag; the descriptor written at a
    buffer of exactly its footprint and not a byte of it at one byte less"""
    p = fixtures()[k]
    for L, name in ((txn.lib(), "fd_txn_parse"), (ref, "ref_txn_parse")):
        first = (ctypes.c_long * 3)()
        nbad = core.core_txn_sweep_cmp(p, len(p), _addr(L, name), first)
        assert nbad == 0, f"{name}: {nbad} payloads differ, first at byte {first[0]} value {first[1]} (check {first[2]})"


def test_core_random_payloads(core, ref):
    """the inputs of test_txn.py's test_random_payloads_vs_reference"""
    rng = np.random.default_rng(11)
    cands = [bytes(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8)) for _ in range(3000)]
    b = corpus.solana_txns(200, seed=4, sig_dist=[1 / 12] * 12, max_sigs_per_txn=12)
    cands += [bytes(b.blob[i * corpus.TXN_MTU:(i + 1) * corpus.TXN_MTU]) for i in range(20)]
    cands += [b"\x01" + b"\x00" * 70000]
    ours, theirs = _addr(txn.lib(), "fd_txn_parse"), _addr(ref, "ref_txn_parse")
    parsed = 0
    for p in cands:
        assert core.core_txn_cmp(p, len(p), ours) == 0
        assert core.core_txn_cmp(p, len(p), theirs) == 0
        parsed += txn.parse_raw(p)[0] != 0
    assert parsed >= 20


def test_core_summary_fields(core):
    f = (ctypes.c_ulong * 6)()
    for p in fixtures():
        t = txn.parse(p)
        assert core.core_txn_summary(p, len(p), f) == t["footprint"]
        assert list(f) == [int.from_bytes(p[1:9], "little"), t["footprint"], 0, t["acct_addr_off"], t["signature_cnt"],
                           t["transaction_version"]]
    p = fixtures()[2]
    assert core.core_txn_summary(p[:-1], len(p) - 1, f) == 0 and list(f)[:2] == [0, 0] and f[2] != 0 and list(f)[3:] == [0, 0, 0xFF]
    assert core.core_txn_summary(b"", 0, f) == 0 and f[2] == 79
    assert core.core_txn_summary(b"\x01" + b"\x00" * 70000, 70001, f) == 0 and f[2] == 73
