"""The slot lifecycle of the engine's synchronous calls (take -> stage ->
enqueue -> settle, fd_ed25519_gpu_host.cpp): every one of the eleven entry
points hands its ring slot back, a call whose wait times out orphans its
slot and the engine recovers, and the two chosen-digest diagnostics are one
code path.

Expected values never come from the engine: the reference build that travels
with the tree (ref_verify_batch, ref_txn_parse through test_gpu_txn.expect,
ref_fe_mul_avx), the host signer (fa.sign_batch), hashlib's SHA-512 and
big-integer arithmetic mod L.  Every comparison is exact.  Slot states are read
through fd_ed25519_gpu_slot_states: bit 1 a ticket, 2 staged, 4 retiring,
8 orphaned."""
import ctypes
import hashlib
import time

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P, oracle_batch
from firedancer_amd import corpus, txn
from test_fe_gpu import rand_fe, ref_mul
from test_gpu_chosen_scalars import set_schedule
from test_gpu_txn import expect, same
from test_gpu_txn_ring import slot_states
from test_sign_host import L, model_base_mul

pytestmark = pytest.mark.gpu

MAX_SIGS, MAX_BLOB, DEPTH = 1 << 12, 1 << 22, 2
BUSY = 1 | 2 | 4 | 8
MTU = corpus.TXN_MTU


def new_engine():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    return fa.Engine(0, MAX_SIGS, MAX_BLOB, depth=DEPTH)


def all_free(eng):
    st = slot_states(eng)
    return len(st) == DEPTH and not any(s & BUSY for s in st)


def digests(b):
    """SHA-512(R || A || M) of every signature of a batch, [n, 64]"""
    return np.array([np.frombuffer(hashlib.sha512(b.sig(i)[:32] + b.pub(i) + b.msg(i)).digest(), np.uint8) for i in range(len(b))])


def k_of(dig):
    return np.array([np.frombuffer((int.from_bytes(d.tobytes(), "little") % L).to_bytes(32, "little"), np.uint8) for d in dig])


# ---------------------------------------------------------------- the five product calls
#
# A Call holds fixed inputs and what they must give.  run(eng, at=None) makes the raw
# call -> (code, outputs); at: the address of a staged blob that already holds self.blob.

class Call:
    def check(self, out):
        assert len(out) == len(self.exp)
        for g, x in zip(out, self.exp):
            assert np.array_equal(g, x)


class Verify(Call):
    def __init__(self, n, ref):
        self.b = corpus.simple(n, msg_sz=96, seed=51)
        self.blob = self.b.blob
        self.exp = (oracle_batch(ref, self.b),)
        assert not self.exp[0].any()

    def run(self, eng, at=None):
        out = np.full(len(self.b), 99, np.int32)
        r = fa.lib().fd_ed25519_gpu_verify_packed(eng._h, len(self.b), P(self.blob), self.blob.nbytes, P(self.b.desc), P(out))
        return r, (out,)


class Sha512(Call):
    def __init__(self, n, ref=None):
        rng = np.random.default_rng(52)
        sz = np.array([(37 * i) % 240 for i in range(n)], np.uint32)        # 0 .. 239 bytes: one and two blocks
        self.desc = np.zeros(n, fa.DESC_DTYPE)
        self.desc["msg_off"] = np.cumsum(sz) - sz
        self.desc["msg_sz"] = sz
        self.blob = rng.integers(0, 256, int(sz.sum()) + 8, dtype=np.uint8)
        self.blob_sz = int(sz.sum())
        self.exp = (np.concatenate([np.frombuffer(hashlib.sha512(self.blob[o:o + s].tobytes()).digest(), np.uint8)
                                    for o, s in zip(self.desc["msg_off"].tolist(), sz.tolist())]),)

    def run(self, eng, at=None):
        n = len(self.desc)
        out = np.zeros(64 * n, np.uint8)
        r = fa.lib().fd_ed25519_gpu_sha512_packed(eng._h, n, at or P(self.blob), self.blob_sz, P(self.desc), P(out), 0)
        return r, (out,)


class Sign(Call):
    MSG = 48

    def __init__(self, n, ref=None):
        rng = np.random.default_rng(53)
        self.seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.blob = np.concatenate([self.seeds.reshape(-1), rng.integers(0, 256, n * self.MSG, dtype=np.uint8)])
        self.desc = np.zeros(n, fa.SIGN_DESC_DTYPE)
        self.desc["seed_off"] = 32 * np.arange(n)
        self.desc["pub_off"] = fa.SIGN_DERIVE
        self.desc["msg_off"] = 32 * n + self.MSG * np.arange(n)
        self.desc["msg_sz"] = self.MSG
        pub, sig = fa.sign_batch(self.seeds, self.blob, self.desc["msg_off"].astype(np.uint64), self.desc["msg_sz"])
        self.exp = (sig, pub, np.zeros(n, np.int32))

    def run(self, eng, at=None):
        n = len(self.desc)
        sig, pub, codes = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8), np.full(n, 99, np.int32)
        r = fa.lib().fd_ed25519_gpu_sign_packed(eng._h, n, at or P(self.blob), self.blob.nbytes, P(self.desc), P(sig), P(pub), P(codes))
        return r, (sig, pub, codes)


class Public(Sign):
    def __init__(self, n, ref=None):
        Sign.__init__(self, n)
        self.exp = (self.exp[1],)

    def run(self, eng, at=None):
        pub = np.zeros((len(self.seeds), 32), np.uint8)
        r = fa.lib().fd_ed25519_gpu_public_packed(eng._h, len(self.seeds), P(self.seeds), P(pub))
        return r, (pub,)


class Txns(Call):
    """n transaction entries over n_sig single-signature payloads (entries may share a payload)"""

    def __init__(self, n, ref, payloads=None):
        b = corpus.solana_txns(payloads or n, seed=54, p2=0.0)
        ps = [bytes(b.blob[i * MTU:(i + 1) * MTU]) for i in range(payloads or n)]
        self.blob, t = txn.pack(ps, gap=1, first=1)
        self.t = t[np.arange(n) % len(t)].copy()
        self.res = expect(ref, self.blob, self.t)[0]
        assert not self.res["status"].any() and (self.res["sig_cnt"] == 1).all()

    def run(self, eng, at=None):
        res = np.zeros(len(self.t), fa.TXN_RESULT_DTYPE)
        r = fa.lib().fd_ed25519_gpu_verify_txns_packed(eng._h, len(self.t), P(self.blob), self.blob.nbytes, P(self.t), P(res), None, None, 0)
        return r, (res,)

    def check(self, out):
        same(out[0], self.res)


# ---------------------------------------------------------------- 1. every slot comes back

def test_every_slot_comes_back(ref):
    """each of the eleven synchronous entry points once at n = 5, its results against
    the reference, and every slot free after each; sha512_packed and sign_packed also
    on a staged blob, which the call consumes; and one refused call per entry point
    (n > max_sigs; the field and scalar diagnostics bound n by 2^20, verify_txns chunks
    any n and is refused by blob_sz > max_blob, debug_txn_descs by sig_cap > max_sigs)"""
    n = 5
    lib = fa.lib()
    eng = new_engine()
    try:
        v = Verify(n, ref)
        b = v.b
        dig = digests(b)
        # --- the five product calls
        for c in (v, Sha512(n), Sign(n), Public(n), Txns(n, ref)):
            r, out = c.run(eng)
            assert r == 0, (type(c).__name__, r, fa.last_error())
            c.check(out)
            assert all_free(eng), (type(c).__name__, slot_states(eng))
        # --- the six diagnostics
        F, G = rand_fe(np.random.default_rng(55), n, 26), rand_fe(np.random.default_rng(56), n, 26)
        assert np.array_equal(eng.debug_fe(0, F, G)[0], ref_mul(ref, F, G))
        assert all_free(eng)
        k, st = eng.debug_k(b.blob, b.desc)
        assert (st == 1).all() and np.array_equal(k, k_of(dig))
        assert all_free(eng)
        codes, k, st = eng.debug_verify_dig(b.blob, b.desc, dig)
        assert np.array_equal(codes, v.exp[0]) and (st == 1).all() and np.array_equal(k, k_of(dig))
        assert all_free(eng)
        s = eng.debug_stages(b.blob, b.desc)
        assert np.array_equal(s.codes, v.exp[0]) and (s.status == 1).all()
        assert all_free(eng)
        sc = np.random.default_rng(57).integers(0, 256, (n, 32), dtype=np.uint8)
        sc[:, 31] &= 0x0F
        got = eng.debug_sign_op(0, sc)
        assert [g.tobytes() for g in got] == [model_base_mul(int.from_bytes(x.tobytes(), "little")) for x in sc]
        assert all_free(eng)
        tx = Txns(n, ref)
        ps = [bytes(tx.blob[o:o + z]) for o, z in zip(tx.t["off"].tolist(), tx.t["sz"].tolist())]
        want = np.concatenate([txn.descs_for(p, int(o)) for p, o in zip(ps, tx.t["off"])])
        desc, n_sig, res = eng.debug_txn_descs(tx.blob, tx.t, len(want))
        assert n_sig == len(want) and np.array_equal(desc, want) and (res["sig_cnt"] == 1).all()
        assert all_free(eng)
        # --- a staged blob: the call consumes the stage
        for c in (Sha512(n), Sign(n)):
            hb, hd = ctypes.c_void_p(0), ctypes.c_void_p(0)
            assert lib.fd_ed25519_gpu_stage(eng._h, ctypes.byref(hb), ctypes.byref(hd)) == 0
            assert sorted(x & BUSY for x in slot_states(eng)) == [0, 2]
            ctypes.memmove(hb.value, c.blob.ctypes.data, c.blob.nbytes)
            r, out = c.run(eng, at=hb)
            assert r == 0, (type(c).__name__, r, fa.last_error())
            c.check(out)
            assert all_free(eng), (type(c).__name__, slot_states(eng))
        # --- refused calls leave every slot free
        big, huge = MAX_SIGS + 1, (1 << 20) + 1
        buf = np.zeros(1 << 16, np.uint8)
        d = np.zeros(8, fa.DESC_DTYPE)
        t = np.zeros(8, fa.TXN_DTYPE)
        cnt = ctypes.c_ulong(0)
        h = eng._h
        refused = {
            "verify_packed": lib.fd_ed25519_gpu_verify_packed(h, big, P(buf), 1024, P(d), P(buf)),
            "debug_fe": lib.fd_ed25519_gpu_debug_fe(h, 0, huge, P(buf), P(buf), P(buf)),
            "debug_k": lib.fd_ed25519_gpu_debug_k(h, big, P(buf), 1024, P(d), P(buf), P(buf)),
            "debug_verify_dig": lib.fd_ed25519_gpu_debug_verify_dig(h, big, P(buf), 1024, P(d), P(buf), P(buf), None, None),
            "debug_stages": lib.fd_ed25519_gpu_debug_stages(h, big, P(buf), 1024, P(d), None, P(buf), *([None] * 8)),
            "sha512_packed": lib.fd_ed25519_gpu_sha512_packed(h, big, P(buf), 1024, P(d), P(buf), 0),
            "sign_packed": lib.fd_ed25519_gpu_sign_packed(h, big, P(buf), 1024, P(d), P(buf), None, P(buf)),
            "public_packed": lib.fd_ed25519_gpu_public_packed(h, big, P(buf), P(buf)),
            "debug_sign_op": lib.fd_ed25519_gpu_debug_sign_op(h, 0, huge, P(buf), None, None, P(buf)),
            "verify_txns_packed": lib.fd_ed25519_gpu_verify_txns_packed(h, 8, P(buf), MAX_BLOB + 1, P(t), P(buf), None, None, 0),
            "debug_txn_descs": lib.fd_ed25519_gpu_debug_txn_descs(h, 8, P(buf), 1024, P(t), big, P(buf), ctypes.byref(cnt), None),
        }
        assert len(refused) == 11 and all(r == fa.ERR_ARG for r in refused.values()), refused
        assert not buf.any()
        assert all_free(eng), slot_states(eng)
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. a timed-out call orphans its slot

@pytest.mark.parametrize("kind", [Verify, Sha512, Sign, Public, Txns], ids=lambda k: k.__name__.lower())
def test_timed_out_call_orphans_its_slot_and_the_engine_recovers(ref, kind):
    """the technique of test_timed_out_calls_do_not_lose_slots (a host wait bound, nothing
    provoked on the device) on each product call at n = 4096 (transactions: 4,096
    entries over 2,048 payloads, as many as the engine's blob holds; 4,096 signatures):
    three calls under a 1 us bound, one more than the ring is deep, each ERR_GPU (timed
    out: its slot is orphaned) or ERR_ARG (both slots orphaned); with the bound
    restored, after 0.2 s, the same call gives the reference's results and every slot
    is free again"""
    c = kind(4096, ref, 2048) if kind is Txns else kind(4096, ref)
    eng = new_engine()
    try:
        old = eng.timeout_ns
        eng.timeout_ns = 1000
        codes, states = [], []
        for _ in range(DEPTH + 1):
            codes.append(c.run(eng)[0])
            states.append(slot_states(eng))
        eng.timeout_ns = old
        print("codes", codes, "states", states)
        assert all(r in (fa.ERR_GPU, fa.ERR_ARG) for r in codes), codes
        assert fa.ERR_GPU in codes, "the 1 us timeout never fired: the test exercised nothing"
        time.sleep(0.2)
        r, out = c.run(eng)
        assert r == 0, (r, fa.last_error())
        c.check(out)
        assert all_free(eng), slot_states(eng)
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. one chosen-digest path

@pytest.mark.parametrize("schedule", ["uniform", "quad", "oct", "pooled"])
def test_debug_verify_dig_and_debug_stages_agree(ref, schedule):
    """codes and status of one batch of five -- three valid rows, a row whose digest is
    not its message's (ERR_MSG) and a descriptor outside the blob (ERR_ARG, status not
    pending) -- from fd_ed25519_gpu_debug_verify_dig and from
    fd_ed25519_gpu_debug_stages( dig ), on every schedule; the valid rows against the
    reference"""
    b = corpus.simple(5, msg_sz=96, seed=58)
    dig = digests(b)
    dig[3] = np.frombuffer(hashlib.sha512(b"another message").digest(), np.uint8)
    desc = b.desc.copy()
    desc[4]["sig_off"] = len(b.blob)
    exp = oracle_batch(ref, b)
    assert not exp.any()
    exp[3], exp[4] = fa.ERR_MSG, fa.ERR_ARG
    eng = new_engine()
    try:
        set_schedule(eng, schedule)
        if schedule == "pooled":
            eng.dsm_pool_min = 1
        codes, _, st = eng.debug_verify_dig(b.blob, desc, dig)
        s = eng.debug_stages(b.blob, desc, dig)
        assert s.schedule == schedule
        assert np.array_equal(codes, s.codes) and np.array_equal(st, s.status), (codes, s.codes, st, s.status)
        assert np.array_equal(codes, exp), (codes, exp)
        assert (st[:4] == 1).all() and st[4] != 1
        assert all_free(eng)
    finally:
        eng.close()
