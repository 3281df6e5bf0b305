"""GPU: the verify front end with the small-order flag read off the encoding
(fd_decomp_body) and the by-one lanes of the cached conversion done without
multiplies (fd_k_dsm_setup, fd_k_dsm), code for code against the reference.

One corpus of 8,197 signatures (not a multiple of 64: the Ai precompute's
partly live last wave): each of the 14 small-order encodings and each of
their 3,584 single-bit flips once as the public key and once as R (random
S < L, 64-byte messages), 998 valid signatures, and the three Q2 vectors,
whose non-canonical limb compare only comes out as the reference's if
every limb of the Ai table is the reference's.  It runs on the quad
schedule (the default at this size), the uniform schedule and the pooled
schedule in AVX mode against the reference build, and once each in strict
and portable mode against their own checkers."""
import random

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import oracle_batch
from firedancer_amd import corpus
from test_portable import codes, refp  # noqa: F401  (refp: the portable reference build)

pytestmark = pytest.mark.gpu

N_VALID = 998


def _flips(encs):
    out = []
    for e in encs:
        for bit in range(256):
            b = bytearray(e)
            b[bit >> 3] ^= 1 << (bit & 7)
            out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def front_corpus():
    smalls = corpus.small_order_encodings()
    encs = smalls + _flips(smalls)
    assert len(encs) == 14 + 3584
    n_enc = len(encs)
    base = corpus.simple(2 * n_enc + N_VALID, 64, seed=4242)
    rnd = random.Random(4242)
    for j, e in enumerate(encs):
        a = np.frombuffer(e, np.uint8)
        # as the public key (R and the message stay a valid signature's)
        po, so = int(base.desc[j]["pub_off"]), int(base.desc[j]["sig_off"])
        base.blob[po:po + 32] = a
        base.blob[so + 32:so + 64] = np.frombuffer(rnd.randrange(corpus.L).to_bytes(32, "little"), np.uint8)
        # as R
        so = int(base.desc[n_enc + j]["sig_off"])
        base.blob[so:so + 32] = a
        base.blob[so + 32:so + 64] = np.frombuffer(rnd.randrange(corpus.L).to_bytes(32, "little"), np.uint8)
    q2 = corpus.from_triples([tuple(bytes.fromhex(h) for h in v) for v in corpus.Q2_VECTORS])
    b = corpus.concat([base, q2])
    assert len(b) == 8197 and len(b) % 64 != 0
    return b


@pytest.fixture(scope="module")
def ref_codes(front_corpus, ref):
    exp = oracle_batch(ref, front_corpus)
    exp.setflags(write=False)
    n_enc = 14 + 3584
    # the corpus really separates the cases: small-order keys and R, points
    # that reach the scalar multiplication, the valid tail, the Q2 rejects
    assert (exp[:14] == fa.ERR_PUBKEY).all() and (exp[n_enc:n_enc + 14] == fa.ERR_SIG).all()
    assert (exp[:n_enc] == fa.ERR_MSG).sum() > 1000 and (exp[n_enc:2 * n_enc] == fa.ERR_MSG).sum() > 1000
    assert (exp[2 * n_enc:2 * n_enc + N_VALID] == fa.SUCCESS).all()
    assert (exp[-3:] == fa.ERR_MSG).all()
    return exp


def _check(got, exp):
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]])


def test_quad_schedule(engine, front_corpus, ref_codes):
    assert engine.mode == fa.MODE_AVX and engine.dsm_oct_max < len(front_corpus) <= engine.dsm_quad_max
    _check(engine.verify_packed(front_corpus.blob, front_corpus.desc), ref_codes)


def test_uniform_schedule(engine, front_corpus, ref_codes):
    quad, oct_, pool = engine.dsm_quad_max, engine.dsm_oct_max, engine.dsm_pool_min
    engine.dsm_pool_min = 1 << 62
    engine.dsm_quad_max = engine.dsm_oct_max = 0
    try:
        got = engine.verify_packed(front_corpus.blob, front_corpus.desc)
    finally:
        engine.dsm_quad_max, engine.dsm_oct_max, engine.dsm_pool_min = quad, oct_, pool
    _check(got, ref_codes)


def test_pooled_schedule(engine, front_corpus, ref_codes):
    pool = engine.dsm_pool_min
    engine.dsm_pool_min = 0
    try:
        got = engine.verify_packed(front_corpus.blob, front_corpus.desc)
    finally:
        engine.dsm_pool_min = pool
    _check(got, ref_codes)


def test_strict_mode(engine, oracle, front_corpus):
    exp = codes(oracle, "oracle_verify_batch_strict", front_corpus)
    engine.mode = fa.MODE_STRICT
    try:
        got = engine.verify_packed(front_corpus.blob, front_corpus.desc)
    finally:
        engine.mode = fa.MODE_AVX
    _check(got, exp)


def test_portable_mode(engine, oracle, refp, front_corpus):  # noqa: F811
    exp = codes(refp, "refp_verify_batch", front_corpus)
    assert (exp == codes(oracle, "oracle_verify_batch_portable", front_corpus)).all()
    engine.mode = fa.MODE_PORTABLE
    try:
        got = engine.verify_packed(front_corpus.blob, front_corpus.desc)
    finally:
        engine.mode = fa.MODE_AVX
    _check(got, exp)
