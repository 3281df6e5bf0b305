"""The signing core (firedancer_amd/csrc/fd_ed25519_gpu_sign_core.h, whose
functions are __host__ __device__) compiled for the host and held against
a big-integer Edwards model written here, the oracle's signer
(oracle_sign / oracle_public_from_private, an independent restatement tied
to the host signer by tests/test_abi.py) and the RFC 8032 7.1 vectors.
Every comparison is exact bytes.  Runs on the CPU: the comb, the recoding,
sc_muladd, the batched inversion and the SHA-512 prefix loader are checked
here before they reach the GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, P, ROOT

PF = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, PF - 2, PF)) % PF


def _inv(x):
    return pow(x, PF - 2, PF)


def _xrecover(y):
    xx = (y * y - 1) * _inv(D * y * y + 1)
    x = pow(xx, (PF + 3) // 8, PF)
    if (x * x - xx) % PF:
        x = x * pow(2, (PF - 1) // 4, PF) % PF
    return PF - x if x & 1 else x


BY = 4 * _inv(5) % PF
B = (_xrecover(BY), BY, 1, _xrecover(BY) * BY % PF)


def ext_add(p, q):
    """extended twisted Edwards addition (a = -1), complete"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % PF, (y1 + x1) * (y2 + x2) % PF
    c, d = 2 * D * t1 * t2 % PF, 2 * z1 * z2 % PF
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % PF, g * h % PF, f * g % PF, e * h % PF


def scalar_mult(s, p=B):
    q = (0, 1, 1, 0)
    while s:
        if s & 1:
            q = ext_add(q, p)
        p = ext_add(p, p)
        s >>= 1
    return q


def encode(p):
    zi = _inv(p[2])
    x, y = p[0] * zi % PF, p[1] * zi % PF
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def model_base_mul(s):
    return encode(scalar_mult(s))


def scalars_to_array(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).reshape(-1, 32).copy()


EDGE_SCALARS = [0, 1, 8, L - 1, L, 2**252,
                int.from_bytes(b"\x88" * 32, "little"),      # every nibble 8: the full recode carry chain
                2**256 - 1,                                   # every nibble 0xF: the carry out of the top digit
                2**255 - 1]                                   # the carry into the top digit

EDGE_TRIPLES = [(0, 0, 0), (L - 1, 2**255 - 8, L - 1), (1, 2**255 - 8, 0), (L - 1, 8, 0), (0, 2**254, L - 1)]


def sign_vectors():
    return json.load(open(os.path.join(GOLDEN, "ed25519_sign_vectors.json")))


def build_harness(out, extra=()):
    src = os.path.join(ROOT, "tests", "sign_host_harness.cpp")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "firedancer_amd", "csrc")]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", *extra, *inc, src, "-o", str(out)],
                   check=True, capture_output=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("signhost") / "signhost.so"
    build_harness(out, ("-O2", "-fPIC", "-shared"))
    H = ctypes.CDLL(str(out))
    H.h_sgn_comb.restype = ctypes.POINTER(ctypes.c_int)
    return H


def h_base_mul(harness, vals):
    s = scalars_to_array(vals)
    out = np.zeros_like(s)
    harness.h_base_mul_enc(P(out), P(s), ctypes.c_ulong(len(s)))
    return out


def limb_value(v):
    x, sh = 0, 0
    for i, t in enumerate(v):
        x += int(t) << sh
        sh += 25 if i & 1 else 26
    return x % PF


def test_comb_table_entries(harness):
    """every entry is the big-integer multiple j 16^i B (and 16^64 B) in cached form"""
    ne, dw = ctypes.c_int(), ctypes.c_int()
    tab = harness.h_sgn_comb(ctypes.byref(ne), ctypes.byref(dw))
    assert (ne.value, dw.value) == (513, 30)
    t = np.ctypeslib.as_array(tab, shape=(513, 3, 10))
    assert np.abs(t).max() <= 1 << 25          # balanced limbs: what fd_sgn_madd's operand ranges assume
    base = B
    for i in range(65):
        m = base
        for j in range(8 if i < 64 else 1):
            zi = _inv(m[2])
            x, y = m[0] * zi % PF, m[1] * zi % PF
            e = t[8 * i + j]
            assert (limb_value(e[0]), limb_value(e[1]), limb_value(e[2])) == ((y + x) % PF, (y - x) % PF, 2 * D * x * y % PF), (i, j)
            if j < 7:
                m = ext_add(m, base)
        base = ext_add(m, m)


def test_base_mul_edges(harness):
    got = h_base_mul(harness, EDGE_SCALARS)
    for s, g in zip(EDGE_SCALARS, got):
        assert g.tobytes() == model_base_mul(s), hex(s)
    assert got[0].tobytes() == b"\x01" + b"\x00" * 31


def test_base_mul_random(harness, oracle):
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
    vals = [int.from_bytes(r.tobytes(), "little") for r in raw]
    got = h_base_mul(harness, vals)
    for s, g in zip(vals, got):
        assert g.tobytes() == model_base_mul(s), hex(s)


def test_base_mul_clamped_vs_oracle(harness, oracle):
    """clamped scalars are what key derivation feeds the comb: [clamp(H(seed))]B is the oracle's public key"""
    rng = np.random.default_rng(2)
    seeds = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    import hashlib
    vals = []
    for sd in seeds:
        h = bytearray(hashlib.sha512(sd.tobytes()).digest()[:32])
        h[0] &= 248
        h[31] &= 63
        h[31] |= 64
        vals.append(int.from_bytes(h, "little"))
    got = h_base_mul(harness, vals)
    for sd, g in zip(seeds, got):
        e = np.zeros(32, np.uint8)
        oracle.oracle_public_from_private(P(e), P(np.ascontiguousarray(sd)))
        assert g.tobytes() == e.tobytes()
        pub = np.zeros(32, np.uint8)
        harness.h_public(P(pub), P(np.ascontiguousarray(sd)))
        assert pub.tobytes() == e.tobytes()


def test_sc_muladd(harness):
    rng = np.random.default_rng(3)
    trip = list(EDGE_TRIPLES)
    for _ in range(3000):
        k, a, r = (int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") for _ in range(3))
        trip.append((k % L, a % 2**255, r % L))
    k, a, r = (scalars_to_array([t[j] for t in trip]) for j in range(3))
    out = np.zeros_like(k)
    harness.h_sc_muladd(P(out), P(k), P(a), P(r), ctypes.c_ulong(len(trip)))
    for t, g in zip(trip, out):
        assert g.tobytes() == ((t[0] * t[1] + t[2]) % L).to_bytes(32, "little"), t


@pytest.mark.parametrize("nact,skipped", [(1, ()), (2, ()), (63, ()), (64, ()), (40, ()), (64, (0, 31, 63)), (64, tuple(range(1, 64)))])
def test_batched_encoding(harness, nact, skipped):
    """Montgomery's trick over a wave, the lane exchange an array: each lane's encoding equals the
    one-inversion one; lanes past nact and rejected lanes hand in 1 and get nothing"""
    rng = np.random.default_rng(nact * 131 + len(skipped))
    raw = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    for i, s in enumerate(EDGE_SCALARS[1:6]):
        raw[i] = scalars_to_array([s])[0]
    skip = np.zeros(64, np.uint8)
    skip[list(skipped)] = 1
    lone = np.zeros_like(raw)
    harness.h_base_mul_enc(P(lone), P(raw), ctypes.c_ulong(64))
    wave = np.zeros_like(raw)
    harness.h_base_mul_enc_wave(P(wave), P(raw), nact, P(skip))
    for l in range(64):
        on = l < nact and not skip[l]
        assert wave[l].tobytes() == (lone[l].tobytes() if on else b"\x00" * 32), l


def h_sign(harness, seed, msg, pub=None):
    sig, pout = np.zeros(64, np.uint8), np.zeros(32, np.uint8)
    m = np.frombuffer(msg, np.uint8).copy() if len(msg) else np.zeros(1, np.uint8)
    s = np.frombuffer(seed, np.uint8).copy()
    pin = None if pub is None else P(np.frombuffer(pub, np.uint8).copy())
    harness.h_sign(P(sig), P(pout), P(s), pin, P(m), ctypes.c_uint32(len(msg)))
    return sig.tobytes(), pout.tobytes()


def test_sign_rfc8032_vectors(harness, oracle):
    for v in sign_vectors():
        seed, pub, msg, sig = (bytes.fromhex(v[k]) for k in ("seed", "pub", "msg", "sig"))
        assert h_sign(harness, seed, msg) == (sig, pub), v["name"]
        assert h_sign(harness, seed, msg, pub) == (sig, pub), v["name"]
        # the fixture itself against the oracle
        e = np.zeros(64, np.uint8)
        m = np.frombuffer(msg, np.uint8).copy() if msg else np.zeros(1, np.uint8)
        oracle.oracle_sign(P(e), P(m), ctypes.c_uint64(len(msg)), P(np.frombuffer(pub, np.uint8).copy()),
                           P(np.frombuffer(seed, np.uint8).copy()))
        assert e.tobytes() == sig, v["name"]


def test_sign_random_vs_oracle(harness, oracle):
    rng = np.random.default_rng(4)
    for i in range(500):
        seed = rng.integers(0, 256, 32, dtype=np.uint8)
        sz = int(rng.integers(0, 301))
        msg = rng.integers(0, 256, max(sz, 1), dtype=np.uint8)
        epub, esig = np.zeros(32, np.uint8), np.zeros(64, np.uint8)
        oracle.oracle_public_from_private(P(epub), P(seed))
        oracle.oracle_sign(P(esig), P(msg), ctypes.c_uint64(sz), P(epub), P(seed))
        assert h_sign(harness, seed.tobytes(), msg[:sz].tobytes()) == (esig.tobytes(), epub.tobytes()), (i, sz)
        if i % 10 == 0:
            # a given key that is not the seed's: used as is (the oracle's bytes for that wrong key)
            wrong = rng.integers(0, 256, 32, dtype=np.uint8)
            oracle.oracle_sign(P(esig), P(msg), ctypes.c_uint64(sz), P(wrong), P(seed))
            assert h_sign(harness, seed.tobytes(), msg[:sz].tobytes(), wrong.tobytes()) == (esig.tobytes(), wrong.tobytes())
