"""The small-order flag read off the encoding
(firedancer_amd/csrc/fd_ed25519_gpu_smallorder.h, compiled for the host)
against the reference's own decision: fd_ed25519_ge_frombytes_vartime_2
followed by fd_ed25519_ge_p3_is_small_order (the [8]P limb test,
src/ballet/ed25519/fd_ed25519_ge.c:21-66), on every encoding the
reference decodes out of

  - the 14 small-order encodings,
  - all 3,584 single-bit flips of them,
  - y + p for y = 2..18 with either sign bit (non-canonical, not small),
  - 20,000 seeded random encodings,

and the constant table against corpus.small_order_encodings().  Runs on
the CPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import P, ROOT
from firedancer_amd import corpus


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("smallorder") / "smallorder.so"
    src = os.path.join(ROOT, "tests", "small_order_harness.cpp")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared",
                    *inc, src, "-o", str(out)], check=True, capture_output=True)
    return ctypes.CDLL(str(out))


def flips(encs):
    out = []
    for e in encs:
        for bit in range(256):
            b = bytearray(e)
            b[bit >> 3] ^= 1 << (bit & 7)
            out.append(bytes(b))
    return out


def classify(harness, encs):
    a = np.frombuffer(b"".join(encs), np.uint8).copy()
    flag = np.zeros(len(encs), np.int32)
    harness.h_enc_is_small_order(P(flag), P(a), ctypes.c_ulong(len(encs)))
    return flag


def reference(ref, encs):
    """(decodes, small order) per encoding from the reference build"""
    dec = np.zeros(len(encs), bool)
    small = np.zeros(len(encs), bool)
    p0, p1 = np.zeros(40, np.int32), np.zeros(40, np.int32)
    for i, e in enumerate(encs):
        s = np.frombuffer(e, np.uint8).copy()
        if ref.ref_ge_frombytes_2(P(p0), P(s), P(p1), P(s)) == 0:
            dec[i] = True
            small[i] = ref.ref_ge_is_small_order(P(p0)) != 0
    return dec, small


def test_table_is_the_small_order_y_fields(harness):
    tab = np.zeros((16, 8), np.uint32)
    n = harness.h_small_order_table(P(tab))
    got = sorted(int.from_bytes(tab[c].tobytes(), "little") for c in range(n))
    exp = sorted({int.from_bytes(e, "little") & ((1 << 255) - 1) for e in corpus.small_order_encodings()})
    assert n == 7 and got == exp


def test_the_14_encodings(harness, ref):
    encs = corpus.small_order_encodings()
    assert len(set(encs)) == 14
    dec, small = reference(ref, encs)
    assert dec.all() and small.all()
    assert classify(harness, encs).all()


def test_single_bit_flips(harness, ref):
    smalls = corpus.small_order_encodings()
    encs = flips(smalls)
    assert len(encs) == 3584
    dec, small = reference(ref, encs)
    got = classify(harness, encs) != 0
    assert dec.sum() > 1000                       # about half of all y are on the curve
    assert (got[dec] == small[dec]).all(), np.nonzero(dec & (got != small))[0][:10]
    # a flip that is flagged landed on another of the 14 (a sign-bit flip, or
    # a neighbour among 0, 1 / p-1, p, p+1)
    assert small[dec].sum() > 0
    assert all(encs[i] in smalls for i in np.nonzero(got)[0])


def test_noncanonical_y_plus_p(harness, ref):
    encs = []
    for y in range(2, 19):
        for s in (0, 1):
            b = bytearray((y + corpus.P).to_bytes(32, "little"))
            b[31] |= s << 7
            encs.append(bytes(b))
    dec, small = reference(ref, encs)
    got = classify(harness, encs) != 0
    assert dec.any()
    assert (got[dec] == small[dec]).all()
    assert not got.any()


def test_random_encodings(harness, ref):
    rng = np.random.default_rng(20240607)
    encs = [rng.bytes(32) for _ in range(20000)]
    dec, small = reference(ref, encs)
    got = classify(harness, encs) != 0
    assert 9000 < dec.sum() < 11000
    assert (got[dec] == small[dec]).all()
    assert not got.any()
