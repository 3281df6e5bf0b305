"""Proof-of-History on the host (include/fd_poh_gpu.h): fd_poh_append,
fd_poh_mixin, fd_poh_verify_batch and fd_poh_gpu_chain against
hashlib.sha256 and the two mainnet vectors of the reference's test
(tests/golden/poh_vectors.json).  No device."""
import hashlib
import re
import os

import numpy as np
import pytest

import firedancer_amd as fa
import poh_grid as pg
from conftest import ROOT


@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_append(n):
    s = bytes(range(1, 33))
    assert fa.poh_append(s, n) == pg.ref(s, n)


def test_mixin():
    s, m = bytes(range(32)), bytes(range(200, 232))
    assert fa.poh_mixin(s, m) == hashlib.sha256(s + m).digest()


def test_vectors():
    for v in pg.vectors():
        s = bytes.fromhex(v["pre"])
        for st in v["steps"]:
            s = fa.poh_append(s, st["n"]) if "n" in st else fa.poh_mixin(s, bytes.fromhex(st["mixin"]))
        assert s.hex() == v["post"], v["name"]


def test_random_states_step_and_mix():
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, (10000, 64), dtype=np.uint8)
    raw[0] = 0
    raw[1] = 255
    for r in raw:
        s, m = r[:32].tobytes(), r[32:].tobytes()
        assert fa.poh_append(s, 1) == hashlib.sha256(s).digest()
        assert fa.poh_mixin(s, m) == hashlib.sha256(s + m).digest()


def test_padding_block_table():
    """FD_POH_KW2_LIST is K[t] + W[t] of the block that only pads a 64-byte message"""
    src = open(os.path.join(ROOT, "firedancer_amd", "csrc", "fd_poh_core.h")).read()

    def words(name):
        body = re.search(r"#define " + name + r" \\\n((?:.*\\\n)*.*)\n", src).group(1)
        return [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})U", body)]
    K, KW = words("FD_POH_K_LIST"), words("FD_POH_KW2_LIST")
    assert len(K) == 64 and len(KW) == 64
    M = 0xffffffff
    rot = lambda x, n: ((x >> n) | (x << (32 - n))) & M  # noqa: E731
    W = [0x80000000] + [0] * 14 + [512]
    for t in range(16, 64):
        s0 = rot(W[t - 15], 7) ^ rot(W[t - 15], 18) ^ (W[t - 15] >> 3)
        s1 = rot(W[t - 2], 17) ^ rot(W[t - 2], 19) ^ (W[t - 2] >> 10)
        W.append((W[t - 16] + s0 + W[t - 7] + s1) & M)
    assert KW == [(k + w) & M for k, w in zip(K, W)]


@pytest.mark.parametrize("C", [1, 4, 64])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("threads", [1, 5])
def test_verify_batch_grid(C, count, threads):
    ent, codes, states = pg.grid(C, count)
    got, st = fa.poh_verify_batch(ent, 2 * C + 1, states=True, nthreads=threads)
    assert (got == codes).all()
    assert (st == states).all()
    assert (fa.poh_verify_batch(ent, 2 * C + 1, nthreads=threads) == codes).all()


def test_verify_batch_err_arg_and_wrong_expect():
    rng = np.random.default_rng(5)
    ent = np.zeros(12, fa.POH_ENTRY_DTYPE)
    for i in range(12):
        pg.entry(ent[i], rng.bytes(32), 3 + i, rng.bytes(32) if i & 1 else None)
    true = ent["expect"].copy()
    exp = np.zeros(12, np.int32)
    ent[1]["flags"] |= 2                       # unknown flag
    ent[4]["_pad"] = 1
    ent[7]["n"] = 41                           # > n_max
    ent[10]["flags"] = 0x80000000
    for i in (1, 4, 7, 10):
        exp[i], true[i] = fa.ERR_ARG, 0
    for i, byte in ((0, 0), (5, 15), (8, 31)):  # one bit wrong
        ent[i]["expect"][byte] ^= 0x10
        exp[i] = fa.POH_ERR_HASH
    got, st = fa.poh_verify_batch(ent, 40, states=True, nthreads=3)
    assert (got == exp).all()
    assert (st == true).all()


def test_verify_batch_args():
    ent = np.zeros(2, fa.POH_ENTRY_DTYPE)
    L = fa.lib()
    out = np.zeros(2, np.int32)
    assert L.fd_poh_verify_batch(2, ent.ctypes.data, 1, out.ctypes.data, None, 0) == fa.ERR_ARG
    assert L.fd_poh_verify_batch(2, ent.ctypes.data, 1, out.ctypes.data, None, 257) == fa.ERR_ARG
    assert L.fd_poh_verify_batch(2, None, 1, out.ctypes.data, None, 1) == fa.ERR_ARG
    assert L.fd_poh_verify_batch(0, None, 1, None, None, 1) == 0


def test_chain():
    rng = np.random.default_rng(3)
    seed = rng.bytes(32)
    hashes = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    ent = np.zeros(9, fa.POH_ENTRY_DTYPE)
    ent["n"] = np.arange(9)
    ent["mixin"][:] = 0x5a
    before = ent.copy()
    fa.poh_chain(seed, hashes, ent)
    assert ent["start"][0].tobytes() == seed
    assert (ent["start"][1:] == hashes[:-1]).all()
    assert (ent["expect"] == hashes).all()
    for f in ("n", "mixin", "flags", "_pad"):
        assert (ent[f] == before[f]).all()


def test_chain_verifies_a_real_run():
    """entries cut from one real chain verify, and a wrong claimed hash fails
    its own entry and its successor's start, no other"""
    s = bytes(32)
    steps = [(5, None), (0, b"\x01" * 32), (17, b"\x02" * 32), (1, None), (9, None)]
    hashes, ent = [], np.zeros(len(steps), fa.POH_ENTRY_DTYPE)
    for i, (n, mx) in enumerate(steps):
        s = pg.ref(s, n, mx)
        hashes.append(np.frombuffer(s, np.uint8))
        ent[i]["n"] = n
        if mx:
            ent[i]["flags"], ent[i]["mixin"] = fa.POH_MIXIN, np.frombuffer(mx, np.uint8)
    hashes = np.array(hashes)
    fa.poh_chain(bytes(32), hashes, ent)
    assert (fa.poh_verify_batch(ent, 100) == 0).all()
    hashes[2, 9] ^= 4
    fa.poh_chain(bytes(32), hashes, ent)
    assert fa.poh_verify_batch(ent, 100).tolist() == [0, 0, fa.POH_ERR_HASH, fa.POH_ERR_HASH, 0]
