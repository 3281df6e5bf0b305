"""Messages longer than the engine's staging blob.

The reference verifies a message of any length (fd_ed25519.h:96-101;
fd_sha512_append streams it, src/ballet/sha512/fd_sha512.c:282-349).  The
engine stages a batch's bytes in a pinned blob of max_blob bytes; a message
that does not fit is hashed on the device in blob-sized pieces with the
SHA-512 chaining state kept in HBM between launches (fd_k_sha512_stream),
then verified by the same prep (digest fed in), decompression and DSM code
as every batch.  Parity: codes equal the reference's own fd_ed25519_verify
(oracle/_ref/libfdref.so) on identical inputs -- valid and corrupted
signatures over 3 MB and 5 MB messages on an engine with a 1 MB blob, at
the short/long boundary, mixed with short messages; through the engine's
pointer-batch API and, in a child process whose default engine has a 1 MB
blob, through fd_ed25519_verify (4 threads), fd_ed25519_verify_batch and
fd_ed25519_verify_batch_single_msg.

The second half runs the same path on engines of 2,048 to 17,920 blob
bytes, where every tail residue of the padded stream, every position of a
piece edge against the end of the message, several groups per call and the
stream kernel's second workgroup cost a few kilobytes each (row h3 of the
DESIGN test table)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import ROOT

MB = 1 << 20
BLOB = MB                       # engine staging blob: the long path starts at BLOB - 96 + 1
LIM = BLOB - 96


def _keypair(rng):
    L = fa.lib()
    priv = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    pub = ctypes.create_string_buffer(32)
    L.fd_ed25519_public_from_private(pub, priv, None)
    return priv, pub.raw


def _sign(msg, priv, pub):
    sig = ctypes.create_string_buffer(64)
    fa.lib().fd_ed25519_sign(sig, msg.ctypes.data if len(msg) else None, len(msg), pub, priv, None)
    return sig.raw


def _cases(seed):
    """(msg uint8 array, sig, pub, what) -- long, boundary and short"""
    rng = np.random.default_rng(seed)
    out = []
    for sz in (3 * MB, 5 * MB, LIM + 1, LIM, 1232 - 65, 0):
        m = rng.integers(0, 256, sz, dtype=np.uint8)
        priv, pub = _keypair(rng)
        sig = _sign(m, priv, pub)
        out.append((m, sig, pub, f"valid {sz}"))
        if sz >= 3 * MB:
            bad = m.copy()
            bad[-1] ^= 0x40                                 # last byte: in the final piece
            out.append((bad, sig, pub, f"msg flip end {sz}"))
            bad2 = m.copy()
            bad2[sz // 2] ^= 1                              # a middle piece
            out.append((bad2, sig, pub, f"msg flip mid {sz}"))
            r = bytearray(sig)
            r[5] ^= 2
            out.append((m, bytes(r), pub, f"R flip {sz}"))
            s = bytearray(sig)
            s[63] = 0xff                                    # S >= L: ERR_SIG before any hash
            out.append((m, bytes(s), pub, f"S>=L {sz}"))
            q1 = bytearray(sig)
            q1[63] = 0x10
            q1[50] |= 1                                     # the reference's early accept
            out.append((m, bytes(q1), pub, f"Q1 {sz}"))
            out.append((m, sig, bytes(32), f"small-order A {sz}"))
            out.append((m, sig, bytes(pub[:31]) + bytes([pub[31] ^ 0x80]), f"A sign flip {sz}"))
    return out


def _expected(ref, cases):
    return np.array([ref.ref_verify(m.ctypes.data if len(m) else None, len(m), s, p) for m, s, p, _ in cases], np.int32)


@pytest.mark.gpu
def test_long_messages_engine_batch_vs_reference(ref):
    cases = _cases(11)
    exp = _expected(ref, cases)
    assert (exp == 0).sum() >= 5 and (exp != 0).sum() >= 8
    eng = fa.Engine(0, 64, BLOB, depth=2)
    try:
        r, got = eng.verify_ptrs([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        bad = [(cases[i][3], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
        assert not bad, bad
        first = exp[exp != 0]
        assert r == (int(first[0]) if len(first) else 0)
        # every mode runs the long path through its own checks: the strict
        # mode still accepts the valid ones and rejects the corrupted
        eng.mode = fa.MODE_STRICT
        r2, got2 = eng.verify_ptrs([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        for (m, s, p, what), g, e in zip(cases, got2, exp):
            if what.startswith("valid"):
                assert g == 0, what
            elif what.startswith(("msg", "R flip")):
                assert g != 0, what
    finally:
        eng.close()


@pytest.mark.gpu
def test_long_messages_reference_drop_ins_vs_reference(ref, tmp_path):
    cases = _cases(12)
    exp = _expected(ref, cases)
    rng = np.random.default_rng(13)
    shared = rng.integers(0, 256, 3 * MB + 17, dtype=np.uint8)
    ssig, spub = [], []
    for k in range(6):
        priv, pub = _keypair(rng)
        ssig.append(_sign(shared, priv, pub))
        spub.append(pub)
    s = bytearray(ssig[3])
    s[9] ^= 4
    ssig[3] = bytes(s)                                      # one corrupted signer
    sexp = np.array([ref.ref_verify(shared.ctypes.data, len(shared), a, b) for a, b in zip(ssig, spub)], np.int32)
    assert (sexp == 0).sum() == 5 and sexp[3] != 0
    npz = tmp_path / "cases.npz"
    np.savez(npz, n=len(cases), sig=np.array([np.frombuffer(c[1], np.uint8) for c in cases]),
             pub=np.array([np.frombuffer(c[2], np.uint8) for c in cases]), shared=shared,
             ssig=np.array([np.frombuffer(x, np.uint8) for x in ssig]), spub=np.array([np.frombuffer(x, np.uint8) for x in spub]),
             **{f"m{i}": c[0] for i, c in enumerate(cases)})
    out = tmp_path / "out.json"
    env = dict(os.environ, FD_ED25519_GPU_DEFAULT_BLOB=str(BLOB), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "long_msg_child.py"), str(npz), str(out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.load(open(out))
    assert got["max_blob"] == BLOB
    names = [c[3] for c in cases]
    assert got["per"] == exp.tolist(), [(n, g, e) for n, g, e in zip(names, got["per"], exp.tolist()) if g != e]
    assert got["batch"] == exp.tolist()
    first = exp[exp != 0]
    assert got["batch_r"] == (int(first[0]) if len(first) else 0)
    assert got["single"] == sexp.tolist() and got["single_r"] == int(sexp[3])


# ---------------------------------------------------------------------------
# The long path on small engines: every tail residue of the padded stream, piece
# edges on and around the end of the message, several groups, lanes that finish
# at different launches, the stream kernel's second workgroup.  With
#   lim = max_blob - 96            (longer messages take the long path)
#   G   = min(max_blob / 256, max_sigs, 4096)        messages per group
#   C   = (max_blob - 16 m) / (128 m)                blocks per message per launch, m in the group
# (fd_run_long), a message's padded stream of P = (64 + sz + 17 + 127) & ~127
# bytes is cut at every multiple of 128 C.  Expected codes are ref_verify's.
SMALL = 2048                    # Engine(0, 64, SMALL): lim = 1952, G = 8; C = 15 at m = 1, 1 at m = 8
TAILS_2 = range(1953, 2081)     # 128 lengths, every residue of (64 + sz) mod 128; 16 or 17 blocks: pieces of 15 + 1 or 15 + 2
TAILS_3 = range(3777, 3905)     # the same residues in three pieces (15 + 15 + 1 or 2)
EDGE_3 = range(3760, 3777)      # 64 + sz = 3824..3840 = 2 * 1920: the cut at 3840 falls between 0x80 and the bit count, and on T


def _valid(rng, sz):
    m = rng.integers(0, 256, sz, dtype=np.uint8)
    priv, pub = _keypair(rng)
    return (m, _sign(m, priv, pub), pub, f"valid {sz}")


def _flip(case, at, what):
    m = case[0].copy()
    m[at] ^= 1 << (at % 8)
    return (m, case[1], case[2], f"{what} of {len(m)}")


def _run(eng, cases):
    return eng.verify_ptrs([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])


def _check(cases, got, exp, r=None):
    bad = [(int(i), cases[i][3], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
    assert not bad, bad[:8]
    if r is not None:
        first = exp[exp != 0]
        assert r == (int(first[0]) if len(first) else 0)


@pytest.fixture(scope="module")
def tails(ref):
    rng = np.random.default_rng(21)
    cases = [_valid(rng, sz) for r_ in (TAILS_2, TAILS_3, EDGE_3) for sz in r_]
    exp = _expected(ref, cases)
    assert (exp == 0).all()             # a condition on the inputs
    assert {(64 + len(c[0])) % 128 for c in cases[:128]} == set(range(128)) == {(64 + len(c[0])) % 128 for c in cases[128:256]}
    return cases, exp


@pytest.fixture(scope="module")
def small_eng():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    eng = fa.Engine(0, 64, SMALL, depth=2)
    yield eng
    eng.mode = fa.MODE_AVX
    eng.close()


@pytest.mark.gpu
def test_small_engine_every_tail_alone(small_eng, tails):
    """one message per call: G = 8, m = 1, C = 15.  Tails of 111 (the padding fits
    exactly), 112..127 (an extra block) and 0 among the 128 residues; for 64 + sz
    > 2031 (> 3951) the last piece holds two blocks; EDGE_3: the second cut (3840) lies
    after 0x80 and before the bit count, and for sz = 3776 on T itself"""
    cases, exp = tails
    for c, e in zip(cases, exp):
        r, got = _run(small_eng, [c])
        assert (r, int(got[0])) == (0, 0) == (int(e), int(e)), c[3]


@pytest.mark.gpu
def test_small_engine_strict_mode(small_eng, tails):
    """G = 8, m = 1, C = 15, strict mode: valid stays 0"""
    cases, _ = tails
    small_eng.mode = fa.MODE_STRICT
    try:
        for c in cases[:16]:
            r, got = _run(small_eng, [c])
            assert (r, int(got[0])) == (0, 0), c[3]
    finally:
        small_eng.mode = fa.MODE_AVX


@pytest.mark.gpu
@pytest.mark.parametrize("lo", [0, 128])
def test_small_engine_128_in_one_call(small_eng, tails, ref, lo):
    """128 messages in one call: G = 8, sixteen groups of m = 8, C = 1 -- a cut at every
    block, so on T (tail 0), between 0x80 and the bit count (tails 112..127) and just
    before both.  Every seventh message carries a flipped bit"""
    cases, _ = tails
    cases = [(_flip(c, len(c[0]) - 1 - 13 * i, "flip") if i % 7 == 3 else c) for i, c in enumerate(cases[lo:lo + 128])]
    exp = _expected(ref, cases)
    assert (exp != 0).sum() == 18 and (exp[exp != 0] == fa.ERR_MSG).all()
    r, got = _run(small_eng, cases)
    _check(cases, got, exp, r)


@pytest.mark.gpu
def test_small_engine_mixed_groups(small_eng, ref):
    """21 messages, lengths cycling 1953, 2016, 6000, 20000, 1900: the four of 1900
    bytes are short and take the ring, the 17 long ones run as groups of m = 8, 8
    (C = 1) and 1 (C = 15); within a group lanes finish after 16, 17, 48 and 157
    launches (nblk == 0 from then on, state kept); results come back in call order"""
    rng = np.random.default_rng(22)
    cases = [_valid(rng, (1953, 2016, 6000, 20000, 1900)[i % 5]) for i in range(21)]
    for i, at in ((2, 5999), (3, 1856), (9, 0), (13, 19999), (16, 64), (20, 1000)):
        cases[i] = _flip(cases[i], at, "flip")
    exp = _expected(ref, cases)
    assert (np.nonzero(exp)[0] == [2, 3, 9, 13, 16, 20]).all()
    r, got = _run(small_eng, cases)
    _check(cases, got, exp, r)


def _flip_rows(rng):
    """for six messages: first byte, last byte, the byte before and at every cut of the
    m = 1 schedule (stream offset 1920 k = message byte 1920 k - 64), S >= L, a
    small-order A"""
    out = []
    for sz in (1953, 2016, 2080, 3777, 6000, 20000):
        c = _valid(rng, sz)
        at = {0, sz - 1} | {128 * 15 * k - 64 - d for k in range(1, 12) for d in (0, 1) if 128 * 15 * k - 64 - d < sz}
        out += [_flip(c, a, f"flip {a}") for a in sorted(at)]
        s = bytearray(c[1])
        s[63] = 0xff
        out.append((c[0], bytes(s), c[2], f"S>=L {sz}"))
        out.append((c[0], c[1], bytes(32), f"small-order A {sz}"))
    return out


@pytest.mark.gpu
def test_small_engine_flips(small_eng, ref):
    """each row alone (G = 8, m = 1, C = 15: the cuts the rows are built for), then all
    in one call (groups of m = 8, C = 1)"""
    cases = _flip_rows(np.random.default_rng(23))
    exp = _expected(ref, cases)
    for c, e in zip(cases, exp):                # conditions on the inputs
        assert e == (fa.ERR_MSG if c[3].startswith("flip") else fa.ERR_SIG if c[3].startswith("S>=L") else fa.ERR_PUBKEY), c[3]
    for c, e in zip(cases, exp):
        r, got = _run(small_eng, [c])
        assert (r, int(got[0])) == (int(e), int(e)), c[3]
    r, got = _run(small_eng, cases)
    _check(cases, got, exp, r)


@pytest.mark.gpu
def test_small_engine_nine_signers_one_message(small_eng, ref):
    """nine signers of one 5,000-byte message, the same pointer nine times: G = 8, so a
    group of m = 8 (C = 1) and one of m = 1 (C = 15); signer 6 corrupted"""
    rng = np.random.default_rng(24)
    m = rng.integers(0, 256, 5000, dtype=np.uint8)
    cases = []
    for k in range(9):
        priv, pub = _keypair(rng)
        cases.append((m, _sign(m, priv, pub), pub, f"signer {k}"))
    s = bytearray(cases[6][1])
    s[9] ^= 4
    cases[6] = (m, bytes(s), cases[6][2], "signer 6, R flipped")
    exp = _expected(ref, cases)
    assert (exp == 0).sum() == 8 and exp[6] != 0
    r, got = _run(small_eng, cases)
    _check(cases, got, exp, r)


@pytest.mark.gpu
@pytest.mark.parametrize("max_sigs,max_blob,sizes,flips", [
    # G = min(8, max_sigs) = 1: three groups of m = 1, C = 15
    (1, 2048, (2000, 2100, 5000), (1,)),
    # max_blob no multiple of 128: lim = 2904, G = 11; 17 long messages: m = 11 (C = 2), then m = 6 (C = 3)
    (64, 3000, tuple(range(2905, 2921)) + (9000,), (4, 16)),
    # G = 70: m = 70 (C = 1: lanes 64..69 in fd_k_sha512_stream's second workgroup), then m = 5 (C = 27)
    (128, 17920, tuple(range(17825, 17900)), (3, 64, 69, 72)),
])
def test_other_small_engines(ref, max_sigs, max_blob, sizes, flips):
    rng = np.random.default_rng(25 + max_sigs)
    assert min(sizes) > max_blob - 96           # all long
    cases = [_valid(rng, sz) for sz in sizes]
    for i in flips:
        cases[i] = _flip(cases[i], len(cases[i][0]) - 1 - 100 * i, "flip")
    exp = _expected(ref, cases)
    assert (np.nonzero(exp)[0] == list(flips)).all()
    eng = fa.Engine(0, max_sigs, max_blob)
    try:
        r, got = _run(eng, cases)
        _check(cases, got, exp, r)
        if max_blob == 3000:                    # each alone as well: m = 1, C = 23
            for c, e in zip(cases, exp):
                r, got = _run(eng, [c])
                assert (r, int(got[0])) == (int(e), int(e)), c[3]
    finally:
        eng.close()
