"""Batch signing and key derivation on the device (fd_k_sign / fd_k_public
through Engine.sign_packed, public_from_seeds, sign_dev, debug_sign_op and
sign_batch_gpu) against the host signer, the oracle's signer, the RFC 8032
7.1 vectors and a big-integer model.  Ed25519 signatures are
deterministic: every comparison is exact bytes."""
import ctypes

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P
from test_sign_host import EDGE_SCALARS, EDGE_TRIPLES, L, model_base_mul, scalars_to_array, sign_vectors

pytestmark = pytest.mark.gpu

# the SHA-512 padding boundaries of both prefixes (32 and 64 bytes), and a full transaction
LENGTHS = [0, 1, 15, 16, 47, 48, 79, 80, 111, 112, 127, 128, 143, 144, 175, 176, 1232]


class Case:
    """n (seed, message) pairs packed at unaligned offsets, lengths mixed inside every wave"""

    def __init__(self, n, seed, given=False):
        rng = np.random.default_rng(seed)
        self.n = n
        self.seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.sz = np.array([LENGTHS[(i * 7 + i // 17) % len(LENGTHS)] for i in range(n)], np.uint32)
        parts, off = [], 1
        self.seed_off, self.pub_off, self.msg_off = (np.zeros(n, np.uint32) for _ in range(3))
        parts.append(np.zeros(1, np.uint8))
        self.pub_in = rng.integers(0, 256, (n, 32), dtype=np.uint8)     # overwritten with real keys by with_keys()
        for i in range(n):
            gap = int(rng.integers(0, 4))
            parts.append(rng.integers(0, 256, gap, dtype=np.uint8)); off += gap
            self.seed_off[i] = off; parts.append(self.seeds[i]); off += 32
            if given:
                gap = int(rng.integers(0, 4))
                parts.append(rng.integers(0, 256, gap, dtype=np.uint8)); off += gap
                self.pub_off[i] = off; parts.append(None); off += 32       # filled below
            gap = int(rng.integers(0, 4))
            parts.append(rng.integers(0, 256, gap, dtype=np.uint8)); off += gap
            self.msg_off[i] = off; parts.append(rng.integers(0, 256, int(self.sz[i]), dtype=np.uint8)); off += int(self.sz[i])
        self.given = given
        self._parts = parts
        self.blob = None
        if not given:
            self._finish()

    def _finish(self):
        self.blob = np.concatenate([p for p in self._parts]).astype(np.uint8)
        self.desc = np.zeros(self.n, fa.SIGN_DESC_DTYPE)
        self.desc["seed_off"] = self.seed_off
        self.desc["pub_off"] = self.pub_off if self.given else fa.SIGN_DERIVE
        self.desc["msg_off"] = self.msg_off
        self.desc["msg_sz"] = self.sz

    def with_keys(self, keys):
        """place the given keys (n x 32) at pub_off"""
        it = iter(np.ascontiguousarray(keys, dtype=np.uint8))
        self._parts = [next(it) if p is None else p for p in self._parts]
        self.pub_in = np.ascontiguousarray(keys, dtype=np.uint8)
        self._finish()
        return self

    def host(self, derive=True):
        """(pub, sig) of the host signer; derive False: with pub_in as the keys"""
        L_ = fa.lib()
        pub = np.zeros((self.n, 32), np.uint8) if derive else self.pub_in.copy()
        sig = np.zeros((self.n, 64), np.uint8)
        off = self.msg_off.astype(np.uint64)
        L_.fd_ed25519_sign_batch(self.n, P(self.seeds), P(self.blob), P(off), P(self.sz), P(pub), P(sig), 8 if derive else -8)
        return pub, sig

    def oracle(self, oracle):
        pub, sig = np.zeros((self.n, 32), np.uint8), np.zeros((self.n, 64), np.uint8)
        off = self.msg_off.astype(np.uint64)
        oracle.oracle_sign_batch(ctypes.c_uint64(self.n), P(self.seeds), P(self.blob), P(off), P(self.sz), P(pub), P(sig), 8)
        return pub, sig


def test_rfc8032_vectors(engine):
    vec = sign_vectors()
    assert [v["name"] for v in vec] == ["TEST 1", "TEST 2", "TEST 3", "TEST 1024", "TEST SHA(abc)"]
    seeds = np.array([list(bytes.fromhex(v["seed"])) for v in vec], np.uint8)
    pubs = np.array([list(bytes.fromhex(v["pub"])) for v in vec], np.uint8)
    sigs = np.array([list(bytes.fromhex(v["sig"])) for v in vec], np.uint8)
    assert (engine.public_from_seeds(seeds) == pubs).all()
    parts, off = [], 0
    d_der, d_giv = np.zeros(len(vec), fa.SIGN_DESC_DTYPE), np.zeros(len(vec), fa.SIGN_DESC_DTYPE)
    for i, v in enumerate(vec):
        m = np.frombuffer(bytes.fromhex(v["msg"]), np.uint8)
        parts += [seeds[i], pubs[i], m, np.zeros(i + 1, np.uint8)]
        for d in (d_der, d_giv):
            d[i]["seed_off"], d[i]["msg_off"], d[i]["msg_sz"] = off, off + 64, len(m)
        d_der[i]["pub_off"], d_giv[i]["pub_off"] = fa.SIGN_DERIVE, off + 32
        off += 64 + len(m) + i + 1
    blob = np.concatenate(parts)
    for d in (d_der, d_giv):
        sig, pub, codes = engine.sign_packed(blob, d)
        assert (codes == 0).all()
        assert (sig == sigs).all() and (pub == pubs).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_parity_host_signer_and_oracle(engine, oracle, n):
    """wave and inversion-group boundaries and one past a 4,096 batch; lengths mixed inside each wave"""
    c = Case(n, 100 + n)
    hpub, hsig = c.host()
    opub, osig = c.oracle(oracle)
    assert (hpub == opub).all() and (hsig == osig).all()
    sig, pub, codes = engine.sign_packed(c.blob, c.desc)
    assert (codes == 0).all()
    assert (pub == hpub).all()
    assert (sig == hsig).all()
    assert (engine.public_from_seeds(c.seeds) == hpub).all()


def test_both_inversions_give_the_same_bytes(engine):
    """the per-lane and the wave-batched point encodings (README, Signing: the A/B)"""
    c = Case(193, 7)
    _, hsig = c.host()
    prev = fa.lib().fd_ed25519_gpu_sign_set_batch_inv(0)
    try:
        for on in (0, 1):
            fa.lib().fd_ed25519_gpu_sign_set_batch_inv(on)
            sig, pub, codes = engine.sign_packed(c.blob, c.desc)
            assert (codes == 0).all() and (sig == hsig).all(), on
            assert (engine.public_from_seeds(c.seeds[:70]) == pub[:70]).all(), on
    finally:
        fa.lib().fd_ed25519_gpu_sign_set_batch_inv(prev)


def test_keys_given_wrong_and_mixed(engine):
    n = 130
    derived, _ = Case(n, 11).host()
    keys = derived.copy()
    rng = np.random.default_rng(12)
    wrong = np.arange(n) % 3 == 1
    keys[wrong] = rng.integers(0, 256, (int(wrong.sum()), 32), dtype=np.uint8)      # not the seeds' keys: used as is
    c = Case(n, 11, given=True).with_keys(keys)
    hpub, hsig = c.host(derive=False)
    sig, pub, codes = engine.sign_packed(c.blob, c.desc)
    assert (codes == 0).all()
    assert (pub == keys).all()                     # pub_out_opt: the key each signature was made with
    assert (sig == hsig).all()
    # derive and given lanes mixed inside one wave
    mix = c.desc.copy()
    der = np.arange(n) % 2 == 0
    mix["pub_off"][der] = fa.SIGN_DERIVE
    sig2, pub2, codes2 = engine.sign_packed(c.blob, mix)
    exp_pub = np.where(der[:, None], derived, keys)
    c.pub_in = exp_pub
    _, hsig2 = c.host(derive=False)
    assert (codes2 == 0).all() and (pub2 == exp_pub).all() and (sig2 == hsig2).all()
    # deterministic: a second run of the same batch gives the same bytes; pub_out_opt may be NULL
    sig3, pub3, _ = engine.sign_packed(c.blob, mix, want_pub=False)
    assert pub3 is None and (sig3 == sig2).all()


def test_out_of_bounds_descriptors(engine):
    c = Case(65, 21, given=True)
    keys, _ = Case(65, 21).host()
    c.with_keys(keys)
    _, hsig = c.host(derive=False)
    d = c.desc.copy()
    sz = len(c.blob)
    d[0]["seed_off"] = sz - 31                     # seed runs one byte past the blob
    d[31]["pub_off"] = sz - 16                     # key past the blob
    d[64]["msg_off"], d[64]["msg_sz"] = sz - 10, 11
    bad = np.zeros(65, bool)
    bad[[0, 31, 64]] = True
    sig, pub, codes = engine.sign_packed(c.blob, d)
    assert (codes[bad] == fa.ERR_ARG).all() and (codes[~bad] == 0).all()
    assert not sig[bad].any() and not pub[bad].any()
    assert (sig[~bad] == hsig[~bad]).all() and (pub[~bad] == keys[~bad]).all()
    # offsets that would wrap a 32-bit sum
    d2 = c.desc.copy()
    d2[5]["msg_off"], d2[5]["msg_sz"] = 0xFFFFFFF0, 0x20
    d2[6]["seed_off"] = 0xFFFFFFFE
    sig, pub, codes = engine.sign_packed(c.blob, d2)
    assert codes[5] == fa.ERR_ARG and codes[6] == fa.ERR_ARG and (np.delete(codes, [5, 6]) == 0).all()
    assert (np.delete(sig, [5, 6], 0) == np.delete(hsig, [5, 6], 0)).all()


def test_malformed_calls_are_err_arg():
    e = fa.Engine(0, 256, 1 << 16, depth=2)
    try:
        L_ = fa.lib()
        buf, d, code = np.zeros(1 << 17, np.uint8), np.zeros(300, fa.SIGN_DESC_DTYPE), np.zeros(300, np.int32)
        out = np.zeros(300 * 64, np.uint8)
        assert L_.fd_ed25519_gpu_sign_packed(e._h, 257, P(buf), 1024, P(d), P(out), None, P(code)) == fa.ERR_ARG      # n > max_sigs
        assert L_.fd_ed25519_gpu_sign_packed(e._h, 4, P(buf), (1 << 16) + 1, P(d), P(out), None, P(code)) == fa.ERR_ARG  # blob_sz > max_blob
        assert L_.fd_ed25519_gpu_sign_packed(e._h, 4, P(buf), 1024, None, P(out), None, P(code)) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_sign_packed(e._h, 4, P(buf), 1024, P(d), None, None, P(code)) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_sign_packed(e._h, 4, P(buf), 1024, P(d), P(out), None, None) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_public_packed(e._h, 257, P(buf), P(out)) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_public_packed(e._h, 4, None, P(out)) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_debug_sign_op(e._h, 2, 1, P(buf), P(buf), P(buf), P(out)) == fa.ERR_ARG
        assert L_.fd_ed25519_gpu_debug_sign_op(e._h, 1, 1, P(buf), None, P(buf), P(out)) == fa.ERR_ARG
        assert not out.any() and not code.any()
    finally:
        e.close()


def test_debug_sign_op_edges(engine):
    """inputs the hash-derived r never lets a signature reach"""
    got = engine.debug_sign_op(0, scalars_to_array(EDGE_SCALARS))
    for s, g in zip(EDGE_SCALARS, got):
        assert g.tobytes() == model_base_mul(s), hex(s)
    assert got[0].tobytes() == b"\x01" + b"\x00" * 31
    rng = np.random.default_rng(31)
    trip = list(EDGE_TRIPLES)
    for _ in range(200):
        k, a, r = (int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") for _ in range(3))
        trip.append((k % L, a % 2**255, r % L))
    out = engine.debug_sign_op(1, *(scalars_to_array([t[j] for t in trip]) for j in range(3)))
    for t, g in zip(trip, out):
        assert g.tobytes() == ((t[0] * t[1] + t[2]) % L).to_bytes(32, "little"), t


def test_round_trip_sign_dev_verify_dev(engine, ref):
    """4,096 messages resident in HBM are signed there; verify descriptors over the result; the
    device and the reference both accept every one"""
    import torch
    n = 4096
    c = Case(n, 41)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)                # the caller's stream: both launches are ordered on it, nothing else is
    st = stream.cuda_stream
    assert st
    d_blob = torch.from_numpy(np.concatenate([c.blob, np.zeros(64, np.uint8)])).to(dev)
    d_sdesc = torch.from_numpy(c.desc.view(np.uint8).copy()).to(dev)
    # one verify blob: the messages' blob, then R||S (64 n) and the keys (32 n)
    base = (len(c.blob) + 64 + 15) & ~15
    d_vblob = torch.zeros(base + 96 * n + 64, dtype=torch.uint8, device=dev)
    d_vblob[:len(c.blob)] = d_blob[:len(c.blob)]
    d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    vdesc = np.zeros(n, fa.DESC_DTYPE)
    vdesc["sig_off"] = base + 64 * np.arange(n)
    vdesc["pub_off"] = base + 64 * n + 32 * np.arange(n)
    vdesc["msg_off"], vdesc["msg_sz"] = c.msg_off, c.sz
    d_vdesc = torch.from_numpy(vdesc.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    sig_ptr = d_vblob.data_ptr() + base
    assert sig_ptr % 16 == 0
    engine.sign_dev(n, d_blob.data_ptr(), len(c.blob), d_sdesc.data_ptr(), sig_ptr, sig_ptr + 64 * n, d_codes.data_ptr(), st)
    engine.verify_dev(n, d_vblob.data_ptr(), base + 96 * n, d_vdesc.data_ptr(), d_out.data_ptr(), st)
    stream.synchronize()
    assert (d_codes.cpu().numpy() == 0).all()
    got = d_out.cpu().numpy()
    assert (got == 0).all()
    vb = d_vblob.cpu().numpy()
    sig = vb[base:base + 64 * n].reshape(n, 64).copy()
    pub = vb[base + 64 * n:base + 96 * n].reshape(n, 32).copy()
    hpub, hsig = c.host()
    assert (sig == hsig).all() and (pub == hpub).all()
    codes = np.full(n, -1, np.int32)
    off = c.msg_off.astype(np.uint64)
    ref.ref_verify_batch(ctypes.c_ulong(n), P(sig), P(pub), P(c.blob), P(off), P(c.sz), P(codes), 8)
    assert (codes == got).all()


def test_sign_batch_gpu_chunks():
    """an engine smaller than the batch in signatures and in blob bytes; a message that fits no blob goes to the host routine"""
    n = 1000
    c = Case(n, 51)
    off = c.msg_off.astype(np.uint64)
    hpub, hsig = fa.sign_batch(c.seeds, c.blob, off, c.sz)
    e = fa.Engine(0, 256, 20000, depth=2)
    try:
        pub, sig = fa.sign_batch_gpu(c.seeds, c.blob, off, c.sz, engine=e)
        assert (pub == hpub).all() and (sig == hsig).all()
    finally:
        e.close()
    e = fa.Engine(0, 64, 1024, depth=2)            # the 1,232-byte messages exceed this engine's blob
    try:
        pub, sig = fa.sign_batch_gpu(c.seeds[:200], c.blob, off[:200], c.sz[:200], engine=e)
        assert (pub == hpub[:200]).all() and (sig == hsig[:200]).all()
    finally:
        e.close()
