"""Proof-of-History test cases shared by the host and the device tests: the
oracle (hashlib.sha256, independent of the library), the golden vectors and
the case grid.  Not a test module."""
import hashlib
import json
import os

import numpy as np

import firedancer_amd as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ref(start: bytes, n: int, mixin=None) -> bytes:
    """fd_poh_append( n ), then fd_poh_mixin if mixin is given, by hashlib"""
    s = bytes(start)
    for _ in range(n):
        s = hashlib.sha256(s).digest()
    if mixin is not None:
        s = hashlib.sha256(s + bytes(mixin)).digest()
    return s


def vectors():
    return json.load(open(os.path.join(GOLDEN, "poh_vectors.json")))["vectors"]


def entry(e, start, n, mixin=None, expect=None, flags=None, pad=0):
    """fill entries[i] (a numpy record); expect None: the true state"""
    e["start"] = np.frombuffer(start, np.uint8)
    e["n"] = n
    e["flags"] = (fa.POH_MIXIN if mixin is not None else 0) if flags is None else flags
    e["_pad"] = pad
    if mixin is not None:
        e["mixin"] = np.frombuffer(mixin, np.uint8)
    e["expect"] = np.frombuffer(ref(start, n, mixin) if expect is None else expect, np.uint8)


def grid_lengths(C: int):
    """the lengths of the issue's grid around a launch size C, ordered so
    that neighbours are as ragged as they get: 0 beside 2C+1"""
    return [0, 2 * C + 1, 1, 2 * C, 2, C + 1, 3, C, max(C - 1, 0)]


def grid(C: int, count: int, seed: int = 1):
    """count entries cycling through grid_lengths(C) x mixin {off, on},
    every 7th with one bit of expect flipped.  Returns (entries, codes,
    states): what hashlib says each entry's code and final state are."""
    rng = np.random.default_rng(seed * 1000003 + C * 131 + count)
    combos = [(n, mx) for mx in (False, True) for n in grid_lengths(C)]
    ent = np.zeros(count, fa.POH_ENTRY_DTYPE)
    codes = np.zeros(count, np.int32)
    states = np.zeros((count, 32), np.uint8)
    shift = 0 if count > 1 else len(combos) - 1 - (C % len(combos))   # a lone entry: a long chain, a different one per C
    for i in range(count):
        n, mx = combos[(i + shift) % len(combos)]
        start = rng.bytes(32)
        mixin = rng.bytes(32) if mx else None
        entry(ent[i], start, n, mixin)
        if not mx:
            ent[i]["mixin"] = np.frombuffer(rng.bytes(32), np.uint8)   # garbage that must not be read
        states[i] = ent[i]["expect"]
        if i % 7 == 3:
            ent[i]["expect"][int(rng.integers(32))] ^= 1 << int(rng.integers(8))
            codes[i] = fa.POH_ERR_HASH
    return ent, codes, states


def block1_entries():
    """mainnet block 1 (tests/golden/poh_vectors.json) as seven entries, one
    per step, the starts computed with hashlib.  Returns (entries, post)."""
    v = vectors()[1]
    s = bytes.fromhex(v["pre"])
    ent = np.zeros(len(v["steps"]), fa.POH_ENTRY_DTYPE)
    for i, st in enumerate(v["steps"]):
        if "n" in st:
            entry(ent[i], s, st["n"])
            s = ref(s, st["n"])
        else:
            mx = bytes.fromhex(st["mixin"])
            entry(ent[i], s, 0, mx)
            s = ref(s, 0, mx)
    assert s.hex() == v["post"]
    return ent, s
