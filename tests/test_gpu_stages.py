"""Every stage of the verify launch as DEVICE output, limb for limb (byte for
byte) against the reference.

The reference's AVX build compares non-canonical limb vectors at the end
(SURVEY section 0, Q2), so the device code has to follow the reference's limb
trajectory, not only its field values.  The other GPU tests hold it to that
through verdicts, where a moved limb shows on about one signature per million;
the limb-level tests of the recoder, the quad step and the field edges run
host compiles, without the value barriers, LDS, DPP and alignbit of the gfx950
code.  Engine.debug_stages (fd_ed25519_gpu_debug_stages, host code only) reads
back what one launch leaves in the HBM working set, and this module compares

  a. the decompressed points (fd_k_decomp, fd_k_front's decomp blocks) with
     ref_ge_frombytes_2 and ref_ge_is_small_order,
  b. the op streams of the three device writers in both layouts with the
     reference's slide in the reference's DSM order (expected_stream of
     tests/test_recode_host.py),
  c. the Ai tables (fd_k_dsm AoS, fd_k_dsm_setup [entry][n]) with the
     reference's [2e+1](-A) at the level of field values (the decode model is
     checked on the CPU, tests/test_stage_models.py),
  d. the pooled DSM's final p1p1 rows, multiplied out as fd_k_dsm_final does,
     with all 30 limbs of ref_ge_dsm(k, -A, S),
  e. a pending signature with S = 0 and k = 0 (the zero digest), whose op
     stream holds no addition.

Every expectation comes from oracle/_ref/libfdref.so and the oracle's
oracle_ge_slide, never from the engine; every comparison is exact equality.
Rows s1-s4 of the table in DESIGN.md section 1."""
import hashlib

import numpy as np
import pytest

import firedancer_amd as fa
from conftest import P
from test_gpu_chosen_scalars import mul_base, ref_reduce, ref_verify_dig, set_schedule
from test_recode_host import expected_stream
from test_stage_models import (E, L, PRIME, cover, fe_val, point_encodings, point_rows, ref_neg_point, ref_table, sqrt_branch,
                               stream_rows, stream_scalars, table_entry_fault, u8)

pytestmark = pytest.mark.gpu

FD_OPS_MAX = 512
PT_OK, PT_BAD, PT_SMALL = 0, 1, 2
STRIDE = 104           # bytes per row of the blobs built here (R || S, A, an 8-byte message)


@pytest.fixture(scope="module")
def eng():
    if fa.device_count() < 1:
        pytest.fail("no gfx950 device visible to a -m gpu test")
    e = fa.Engine(0, 4096, 1 << 20)
    yield e
    e.close()


@pytest.fixture
def sched(eng):
    yield lambda name: set_schedule(eng, name)
    set_schedule(eng, "default")
    eng.mode = fa.MODE_AVX


def window(blob, desc, lo, hi, stride=STRIDE):
    """rows [lo, hi) of a blob laid out at `stride` bytes per row, as a batch of their own"""
    d = desc[lo:hi].copy()
    for f in ("sig_off", "pub_off", "msg_off"):
        d[f] -= stride * lo
    b = np.zeros(stride * (hi - lo) + 64, np.uint8)
    b[:stride * (hi - lo)] = blob[stride * lo:stride * hi]
    return b, d


def first_bad(mask):
    return [int(i) for i in np.nonzero(mask)[0][:6]]


# ------------------------------------------------------------ a. points
class PointRef:
    pass


@pytest.fixture(scope="module")
def points(ref):
    c = point_encodings()
    r = PointRef()
    r.blob, r.desc, r.dig = point_rows(c)
    n = r.n = len(r.desc)
    r.pts = np.zeros((2, n, 40), np.int32)            # [A / R][row][40]
    r.pstat = np.zeros((2, n), np.int32)
    r.rejected_by_arithmetic = sum(b is None for b in c.branch)
    for i in range(n):
        enc = (u8(c.enc[2 * i]), u8(c.enc[2 * i + 1]))        # A, R
        a, b = np.zeros(40, np.int32), np.zeros(40, np.int32)
        if ref.ref_ge_frombytes_2(P(a), P(enc[0]), P(b), P(enc[1])) == 0:
            got = [a, b]
        else:
            # one of the two failed: the survivor, if any, paired with itself
            got = []
            for e in enc:
                x, y = np.zeros(40, np.int32), np.zeros(40, np.int32)
                got.append(x if ref.ref_ge_frombytes_2(P(x), P(e), P(y), P(e)) == 0 else None)
        for h in (0, 1):
            if got[h] is None:
                r.pstat[h, i] = PT_BAD
            else:
                r.pts[h, i] = got[h]
                r.pstat[h, i] = PT_SMALL if ref.ref_ge_is_small_order(P(got[h])) else PT_OK
    # conditions on the inputs: the reference rejects exactly the encodings integer
    # arithmetic finds off the curve, and flags the 14 small-order encodings
    bad = (r.pstat == PT_BAD)
    assert int(bad.sum()) == r.rejected_by_arithmetic > 0
    assert [bool(x) for x in bad.T.reshape(-1)] == [b is None for b in c.branch]
    small = {c.enc[2 * i + h] for h in (0, 1) for i in range(n) if r.pstat[h, i] == PT_SMALL}
    assert len(small) == 14
    return r


@pytest.mark.parametrize("front", ["uniform_hash", "quad_hash", "quad_dig"])
def test_points(eng, sched, points, front):
    """X, Y, Z, T of every point the reference decodes and the BAD / SMALL / OK status of
    every point, on the uniform front (fd_k_prep's status, fd_k_decomp), the latency
    front by real hash (fd_k_front's decomp blocks) and by digest (fd_k_decomp with no
    status), in batches of 257, 255 and 1 signatures (the 256-thread block edge of the
    2n grid).  Left out: the points the corpus was built to have rejected, nothing else."""
    r = points
    name = front.split("_")[0]
    sched(name)
    compared = np.zeros((2, r.n), bool)
    left_out = np.zeros((2, r.n), bool)
    sizes = set()
    for lo, hi in cover(r.n, (1, 255, 257)):
        n = hi - lo
        sizes.add(n)
        b, d = window(r.blob, r.desc, lo, hi)
        s = eng.debug_stages(b, d, r.dig[lo:hi] if front == "quad_dig" else None)
        assert s.schedule == name and s.ops_sigmajor == (name == "quad")
        assert (s.status == 1).all(), (front, lo, first_bad(s.status != 1))
        exp_stat = np.concatenate([r.pstat[0, lo:hi], r.pstat[1, lo:hi]])
        exp_pts = np.concatenate([r.pts[0, lo:hi], r.pts[1, lo:hi]])
        assert (s.pstat == exp_stat).all(), (front, lo, n, first_bad(s.pstat != exp_stat))
        ok = exp_stat != PT_BAD
        diff = (s.pts != exp_pts).any(axis=1) & ok
        j = first_bad(diff)
        assert not j, (front, "row", lo + j[0] % n, "AR"[j[0] // n], "limbs", first_bad(s.pts[j[0]] != exp_pts[j[0]]),
                       s.pts[j[0]].tolist(), exp_pts[j[0]].tolist())
        compared[0, lo:hi] |= ok[:n]
        compared[1, lo:hi] |= ok[n:]
        left_out[0, lo:hi] |= ~ok[:n]
        left_out[1, lo:hi] |= ~ok[n:]
    assert sizes == {1, 255, 257}
    assert not (compared & left_out).any() and (compared | left_out).all()
    print(f"points[{front}]: compared {int(compared.sum())}, left out {int(left_out.sum())} (rejected encodings)")
    assert int(left_out.sum()) == r.rejected_by_arithmetic
    assert int(compared.sum()) == 2 * r.n - r.rejected_by_arithmetic


# ------------------------------------------------------------ b. op streams
class StreamRef:
    pass


@pytest.fixture(scope="module")
def streams(ref, oracle):
    pairs = stream_scalars()
    # A and R: two ordinary points (multiples of the base point by the reference's DSM)
    pub, r_enc = mul_base(ref, 0x1234567), mul_base(ref, 0x7654321)
    r = StreamRef()
    r.pairs = pairs
    r.blob, r.desc, r.dig, r.khash = stream_rows(pairs, pub, r_enc)
    n = r.n = len(pairs)
    for i in range(n):              # the k of the hashed rows is the reference's reduction of the real hash
        h = hashlib.sha512(bytes(r.blob[STRIDE * i:STRIDE * i + 32]) + pub + bytes(r.blob[STRIDE * i + 96:STRIDE * i + 104])).digest()
        assert int.from_bytes(ref_reduce(ref, h).tobytes(), "little") == r.khash[i]
    r.exp = {}
    for kind, ks in (("dig", [k for _, k in pairs]), ("hash", r.khash)):
        ops = np.zeros((n, FD_OPS_MAX), np.uint8)
        start = np.zeros(n, np.int32)
        for i, ((S, _), k) in enumerate(zip(pairs, ks)):
            ops[i], start[i] = expected_stream(oracle, S, k)
        r.exp[kind] = (ops, start)
    return r


STREAM_CASES = [("uniform", "hash", (1, 63, 65, 257)), ("uniform", "dig", (1, 63, 65, 257)),
                ("pooled", "hash", (1, 63, 65, 257)), ("pooled", "dig", (1, 63, 65, 257)),
                ("quad", "dig", (1, 17)), ("quad", "hash", (1, 31, 32, 33, 65))]


@pytest.mark.parametrize("schedule,kind,sizes", STREAM_CASES, ids=[f"{a}-{b}" for a, b, _ in STREAM_CASES])
def test_op_streams(eng, sched, streams, schedule, kind, sizes):
    """op_start and all 512 op bytes of every pending row: step-major through fd_k_prep
    (hash) and fd_k_prep_dig, signature-major through fd_k_prep_dig and through
    fd_k_front (fd_prep2_body).  The hashed batches of at most 32 signatures run three
    times back to back: the launch tag changes, and whether the S digits recoded ahead
    (sdig) were taken or the two-pass recoder ran, the bytes are the reference's."""
    r = streams
    sched(schedule)
    exp_ops, exp_start = r.exp[kind]
    compared = np.zeros(r.n, bool)
    not_pending = np.zeros(r.n, bool)
    used = set()
    for lo, hi in cover(r.n, sizes):
        n = hi - lo
        used.add(n)
        b, d = window(r.blob, r.desc, lo, hi)
        for rep in range(3 if (kind == "hash" and schedule == "quad" and n <= 32) else 1):
            s = eng.debug_stages(b, d, r.dig[lo:hi] if kind == "dig" else None)
            assert s.schedule == schedule and s.ops_sigmajor == (schedule == "quad")
            pend = s.status == 1
            assert (s.op_start[~pend] == FD_OPS_MAX).all()
            bad = pend & (s.op_start != exp_start[lo:hi])
            assert not bad.any(), (schedule, kind, n, rep, "op_start, row", lo + first_bad(bad)[0],
                                   int(s.op_start[first_bad(bad)[0]]), int(exp_start[lo + first_bad(bad)[0]]))
            bad = pend & (s.ops != exp_ops[lo:hi]).any(axis=1)
            j = first_bad(bad)
            assert not j, (schedule, kind, n, rep, "ops, row", lo + j[0], "S, k", hex(r.pairs[lo + j[0]][0]),
                           "bytes", first_bad(s.ops[j[0]] != exp_ops[lo + j[0]]))
            compared[lo:hi] |= pend
            not_pending[lo:hi] |= ~pend
    assert used == set(sizes)
    assert not (compared & not_pending).any() and (compared | not_pending).all()
    print(f"op streams[{schedule}-{kind}]: compared {int(compared.sum())}, left out {int(not_pending.sum())} (not pending)")
    assert compared.sum() >= 0.9 * r.n


# ------------------------------------------------------------ c. Ai tables
class TableRef:
    pass


@pytest.fixture(scope="module")
def tables(ref):
    rng = np.random.default_rng(31337)
    encs = []
    while len(encs) < 2 * 513:
        e = bytes(rng.bytes(32))
        if int.from_bytes(e, "little") & ((1 << 255) - 1) < PRIME and sqrt_branch(e) is not None:
            encs.append(e)
    n = 513
    r = TableRef()
    r.n = n
    r.blob = np.zeros(STRIDE * n + 64, np.uint8)
    for i in range(n):
        S = int.from_bytes(rng.bytes(32), "little") % L
        r.blob[STRIDE * i:STRIDE * i + 96] = u8(encs[2 * i + 1] + S.to_bytes(32, "little") + encs[2 * i])
    r.desc = np.zeros(n, fa.DESC_DTYPE)
    r.desc["sig_off"] = STRIDE * np.arange(n)
    r.desc["pub_off"] = STRIDE * np.arange(n) + 64
    r.desc["msg_off"] = STRIDE * np.arange(n) + 96
    r.dig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    r.exp = np.stack([ref_table(ref, encs[2 * i]) for i in range(n)])       # [n][8][30]
    return r


@pytest.mark.parametrize("n", [1, 129, 513])
@pytest.mark.parametrize("schedule", ["uniform", "pooled"])
def test_ai_tables(eng, sched, tables, schedule, n):
    """the four lanes of entry e of every pending signature decode to the cached form of
    the reference's [2e+1](-A), both pad dwords of every lane 0: fd_k_dsm's table (AoS
    per signature) and fd_k_dsm_setup's ([entry][n], stored through LDS in whole waves)"""
    r = tables
    sched(schedule)
    b, d = window(r.blob, r.desc, 0, n)
    s = eng.debug_stages(b, d, r.dig[:n])
    assert s.schedule == schedule and s.tab is not None and s.tab.shape == (n, 8, 4, 12)
    pend = (s.status == 1) & (s.pstat[:n] == PT_OK) & (s.pstat[n:] == PT_OK)
    assert pend.all()          # ordinary points, S < L: nothing is left out
    assert not s.tab[:, :, :, 10:].any(), ("pad dword, (row, entry, lane)", np.argwhere(s.tab[:, :, :, 10:].any(axis=3))[:4].tolist())
    faults = [(i, e, f) for i in range(n) for e in range(8) for f in [table_entry_fault(s.tab[i, e], r.exp[i, e])] if f]
    print(f"Ai tables[{schedule}-{n}]: compared {8 * n} entries of {n} signatures, left out 0")
    assert not faults, (schedule, n, len(faults), faults[:4])


# ------------------------------------------------------------ d. pooled final states
class FinRef:
    pass


@pytest.fixture(scope="module")
def finals(ref):
    rng = np.random.default_rng(777)
    keys = [int.from_bytes(rng.bytes(32), "little") % L for _ in range(3)]
    pubs = [mul_base(ref, a) for a in keys]
    nega = [ref_neg_point(ref, p) for p in pubs]
    grid = [(S, k) for S in E for k in E if (S, k) != (0, 0)]       # (0, 0): R would be the identity
    rnd = [(int.from_bytes(rng.bytes(32), "little") % L, int.from_bytes(rng.bytes(32), "little") % L) for _ in range(256)]
    rows = []                                                       # (valid, key, sig, k)
    for i, (S, k) in enumerate(grid + rnd):
        j = i % 3
        sig = mul_base(ref, (S - k * keys[j]) % L) + S.to_bytes(32, "little")
        rows.append((1, j, sig, k))
        if i < len(grid):
            rows.append((0, j, sig, (k + 1) % L))                   # the same row with k + 1
    perm = np.random.default_rng(5).permutation(len(rows))
    rows = [rows[i] for i in perm]
    n = len(rows)
    r = FinRef()
    r.n = n
    r.valid = np.array([x[0] for x in rows], bool)
    r.blob = np.zeros(STRIDE * n + 64, np.uint8)
    r.dig = np.zeros((n, 64), np.uint8)
    r.exp = np.zeros((n, 30), np.int32)
    r.code = np.zeros(n, np.int32)
    for i, (_, j, sig, k) in enumerate(rows):
        r.blob[STRIDE * i:STRIDE * i + 96] = u8(sig + pubs[j])
        r.dig[i] = u8(k.to_bytes(64, "little"))
        o = np.zeros(30, np.int32)
        ref.ref_ge_dsm(P(o), P(u8(k.to_bytes(32, "little"))), P(nega[j]), P(u8(sig[32:])))
        r.exp[i] = o
        r.code[i] = ref_verify_dig(ref, r.dig[i].tobytes(), sig, pubs[j])
    r.desc = np.zeros(n, fa.DESC_DTYPE)
    r.desc["sig_off"] = STRIDE * np.arange(n)
    r.desc["pub_off"] = STRIDE * np.arange(n) + 64
    r.desc["msg_off"] = STRIDE * np.arange(n) + 96
    r.nega = nega
    r.key = np.array([x[1] for x in rows])
    # conditions on the inputs: 575 + 256 valid rows, 575 wrong ones, by the reference (a
    # valid row the reference refuses through a Q2 limb alias would show here: none does)
    assert n == 2 * 575 + 256 and n >= 1100
    assert (r.code[r.valid] == fa.SUCCESS).all() and (r.code[~r.valid] == fa.ERR_MSG).all()
    return r


def fin_to_p2(ref, fin):
    """X = l0 l3, Y = l1 l2, Z = l2 l3 of final p1p1 rows, by the reference's product (as fd_k_dsm_final)"""
    out = np.zeros((len(fin), 30), np.int32)
    for i, row in enumerate(fin):
        l = [np.ascontiguousarray(row[10 * q:10 * q + 10]) for q in range(4)]
        for o, (f, g) in enumerate(((l[0], l[3]), (l[1], l[2]), (l[2], l[3]))):
            h = np.zeros(10, np.int32)
            ref.ref_fe_mul_avx(P(h), P(f), P(g))
            out[i, 10 * o:10 * o + 10] = h
    return out


@pytest.mark.parametrize("n", [1, 127, 129, 513, 1100])
def test_pool_final_states(eng, sched, finals, ref, n):
    """the pooled DSM's final p1p1 row of every signature, multiplied out, is the
    reference's [k](-A) + [S]B in all 30 limbs: one pool, one past it, the four-wave
    block edge, a ragged last wave under the sg = gw + s nwaves mapping"""
    r = finals
    sched("pooled")
    b, d = window(r.blob, r.desc, 0, n)
    s = eng.debug_stages(b, d, r.dig[:n])
    assert s.schedule == "pooled" and s.fin is not None and not s.ops_sigmajor
    assert (s.status == 1).all() and (s.pstat == PT_OK).all()
    got = fin_to_p2(ref, s.fin)
    bad = (got != r.exp[:n]).any(axis=1)
    j = first_bad(bad)
    print(f"pool finals[{n}]: compared {n}, left out 0")
    assert not j, (n, "row", j[0], "of", int(bad.sum()), "limbs", first_bad(got[j[0]] != r.exp[j[0]]), s.fin[j[0]].tolist())
    assert (s.codes == r.code[:n]).all(), (n, first_bad(s.codes != r.code[:n]))


def test_fin_only_on_pooled(eng, sched, finals):
    for name in ("uniform", "quad", "oct"):
        sched(name)
        b, d = window(finals.blob, finals.desc, 0, 17)
        s = eng.debug_stages(b, d, finals.dig[:17])
        assert s.schedule == name and s.fin is None and (s.tab is not None) == (name == "uniform")
        assert (s.codes == finals.code[:17]).all()
    sched("default")
    for n, name in ((17, "oct"), (64, "oct"), (65, "quad")):
        b, d = window(finals.blob, finals.desc, 0, n)
        assert eng.debug_stages(b, d).schedule == name


# ------------------------------------------------------------ e. the empty stream
def test_zero_scalars_after_a_valid_launch(eng, sched, finals, ref, oracle):
    """S = 0 with the zero digest (k = 0): a pending signature with no addition in its
    stream; [0](-A) + [0]B is the identity, R is not, so the reference says ERR_MSG.
    Launch 1 leaves a valid signature's final state in the same row of the working set;
    launch 2 must not find it.  (The recoder gives such a row op_start = 256, the 256
    doublings, not FD_OPS_MAX: the pool steps it like any other and writes its row.)"""
    r = finals
    n = 129
    rows = np.nonzero(r.valid)[0][:n]
    blob = np.zeros(STRIDE * n + 64, np.uint8)
    for i, g in enumerate(rows):
        blob[STRIDE * i:STRIDE * (i + 1)] = r.blob[STRIDE * g:STRIDE * (g + 1)]
    desc = r.desc[:n]
    dig = r.dig[rows].copy()
    z = 77
    blob2, dig2 = blob.copy(), dig.copy()
    blob2[STRIDE * z + 32:STRIDE * z + 64] = 0          # S = 0, R as it was
    dig2[z] = 0
    sig_z, pub_z = bytes(blob2[STRIDE * z:STRIDE * z + 64]), bytes(blob2[STRIDE * z + 64:STRIDE * z + 96])
    want = np.zeros(n, np.int32)
    want[z] = fa.ERR_MSG
    # conditions on the inputs
    assert ref_verify_dig(ref, bytes(64), sig_z, pub_z) == fa.ERR_MSG
    exp_ops, exp_start = expected_stream(oracle, 0, 0)
    assert exp_start == 256 and not exp_ops.any()

    sched("pooled")
    s1 = eng.debug_stages(blob, desc, dig)
    assert s1.schedule == "pooled" and (s1.codes == fa.SUCCESS).all()
    s2 = eng.debug_stages(blob2, desc, dig2)
    assert s2.schedule == "pooled" and (s2.status == 1).all()
    assert s2.op_start[z] == exp_start and (s2.ops[z] == exp_ops).all()
    ident = np.zeros(30, np.int32)
    ref.ref_ge_dsm(P(ident), P(np.zeros(32, np.uint8)), P(r.nega[r.key[rows[z]]]), P(np.zeros(32, np.uint8)))
    assert (fin_to_p2(ref, s2.fin[z:z + 1])[0] == ident).all(), s2.fin[z].tolist()
    assert fe_val(ident[0:10]) == 0 and fe_val(ident[10:20]) == fe_val(ident[20:30]) != 0
    assert (s2.codes == want).all(), ("pooled", int(s2.codes[z]), first_bad(s2.codes != want))
    for name in ("uniform", "quad", "oct"):
        sched(name)
        assert (eng.debug_stages(blob, desc, dig).codes == fa.SUCCESS).all(), name
        s = eng.debug_stages(blob2, desc, dig2)
        assert s.schedule == name and s.op_start[z] == exp_start and (s.ops[z] == exp_ops).all()
        assert (s.codes == want).all(), (name, int(s.codes[z]), first_bad(s.codes != want))
        codes, _, _ = eng.debug_verify_dig(blob2, desc, dig2)
        assert (codes == want).all(), name


# ------------------------------------------------------------ arguments
def test_stages_args(eng, finals):
    n = 16
    blob, desc = window(finals.blob, finals.desc, 0, n)
    dig = finals.dig[:n]
    with pytest.raises(fa.EngineError):
        eng.debug_stages(blob, desc, dig[:n - 1])                                  # 64 bytes per signature
    with pytest.raises(fa.EngineError):
        eng.debug_stages(blob, np.tile(desc, 512), np.tile(dig, (512, 1)))         # n > max_sigs
    with pytest.raises(fa.EngineError):
        eng.debug_stages(np.zeros(eng.max_blob + 1, np.uint8), desc, dig)          # blob_sz > max_blob
    L_ = fa.lib()
    outs = [np.full(k, 0x55, np.uint8) for k in (4 * n, 4 * n, 8 * n, 320 * n, 4 * n, 512 * n, 1536 * n, 160 * n, 16)]
    po = [fa._p(o) for o in outs]
    dg = np.ascontiguousarray(dig)
    for args in ((None, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dg)),                   # NULL engine
                 (eng._h, eng.max_sigs + 1, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dg)),   # n > max_sigs
                 (eng._h, n, fa._p(blob), eng.max_blob + 1, fa._p(desc), fa._p(dg)),             # blob_sz > max_blob
                 (eng._h, n, fa._p(blob), blob.nbytes, None, fa._p(dg)),                         # NULL desc, n > 0
                 (eng._h, n, None, blob.nbytes, fa._p(desc), fa._p(dg))):                        # NULL blob, blob_sz > 0
        assert L_.fd_ed25519_gpu_debug_stages(*args, *po) == fa.ERR_ARG
    # n == 0 returns 0 and writes nothing, whatever else is NULL
    assert L_.fd_ed25519_gpu_debug_stages(eng._h, 0, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dg), *po) == 0
    assert L_.fd_ed25519_gpu_debug_stages(eng._h, 0, None, 0, None, None, *po) == 0
    assert all((o == 0x55).all() for o in outs)
    s = eng.debug_stages(blob, desc[:0], dig[:0])
    assert s.codes.shape == (0,) and s.pts.shape == (0, 40) and s.ops.shape == (0, 512)
    # every output is optional
    assert L_.fd_ed25519_gpu_debug_stages(eng._h, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dg), *([None] * 9)) == 0
    codes = np.full(n, 99, np.int32)
    assert L_.fd_ed25519_gpu_debug_stages(eng._h, n, fa._p(blob), blob.nbytes, fa._p(desc), fa._p(dg), fa._p(codes), *([None] * 8)) == 0
    assert (codes == finals.code[:n]).all()
    # a descriptor outside the blob: ERR_ARG at that row only, no stream, and its points are not decoded
    d2 = desc.copy()
    d2["pub_off"][5] = blob.nbytes - 31
    s = eng.debug_stages(blob, d2, dig)
    exp = finals.code[:n].copy()
    exp[5] = fa.ERR_ARG
    assert (s.codes == exp).all() and s.status[5] == fa.ERR_ARG and s.op_start[5] == FD_OPS_MAX
