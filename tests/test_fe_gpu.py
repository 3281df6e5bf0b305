"""The engine's field products as DEVICE code (fd_k_debug_fe: the same
fd_ed25519_gpu_fe.h functions the kernels are built from, compiled for
gfx950 with their value barriers) compared limb for limb with the
reference's AVX field ops (oracle/_ref build: FE_AVX_INL_MUL and SQN,
src/ballet/ed25519/avx/fd_ed25519_fe_avx_inl.h:484-677), over the operand
ranges the verify path produces and past them (28-bit limbs exercise the
mod-2^32 operand pre-scales).  tests/test_fe_host.py checks the host
compile of the same functions; end-to-end parity checks them only through
verdicts.  The carry-boundary limbs of test_fe_host.py's
test_carry_edges_vs_oracle (0, +-1, +-2^24, 2^24-1, +-2^25, 2^25-1, 2^26-1,
-2^26) run here too, mixed at random and one-hot.  Row a8 of SURVEY.md
section 8."""
import numpy as np
import pytest

from conftest import P

pytestmark = pytest.mark.gpu

N = 4096


def rand_fe(rng, n, bits):
    return rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, 10), dtype=np.int64).astype(np.int32)


def ref_mul(ref, F, G):
    out = np.zeros_like(F)
    for i in range(len(F)):
        e = np.zeros(10, np.int32)
        ref.ref_fe_mul_avx(P(e), P(np.ascontiguousarray(F[i])), P(np.ascontiguousarray(G[i])))
        out[i] = e
    return out


def ref_sqn(ref, F, n):
    out = np.zeros_like(F)
    for i in range(len(F)):
        e = np.zeros(10, np.int32)
        ref.ref_fe_sqn_avx(P(e), P(np.ascontiguousarray(F[i])), n)
        out[i] = e
    return out


@pytest.mark.parametrize("bits", [25, 26, 27, 28])
def test_device_field_products_vs_reference(engine, ref, bits):
    rng = np.random.default_rng(100 + bits)
    F, G = rand_fe(rng, N, bits), rand_fe(rng, N, bits)
    fg, gf, ff = ref_mul(ref, F, G), ref_mul(ref, G, F), ref_mul(ref, F, F)
    f2, g2x2 = ref_sqn(ref, F, 1), ref_sqn(ref, G, 2)
    f2x2 = ref_sqn(ref, F, 2)
    H = {op: engine.debug_fe(op, F, G) for op in range(8)}
    assert (H[0][0] == fg).all(), "fd_fe_mul"
    assert (H[1][0] == f2).all(), "fd_fe_sqn n=1"
    assert (H[2][0] == f2x2).all(), "fd_fe_sqn n=2"
    assert (H[3][0] == fg).all(), "fd_fe_mul_ilp"
    assert (H[4][0] == fg).all() and (H[4][1] == gf).all(), "fd_fe_mul2"
    assert (H[5][0] == fg).all() and (H[5][1] == gf).all() and (H[5][2] == ff).all(), "fd_fe_chain3"
    assert (H[6][0] == f2).all() and (H[6][1] == g2x2).all(), "fd_fe_sqn2"
    bad = np.nonzero((H[7][0] != fg).any(axis=1))[0]
    assert len(bad) == 0, ("fd_o_mul (oct DSM half product)", bad[:8], H[7][0][bad[:2]], fg[bad[:2]])


def check_all_ops(engine, ref, F, G, what):
    """the eight debug_fe ops on the pairs (F, G) against the reference, as above"""
    fg, gf, ff = ref_mul(ref, F, G), ref_mul(ref, G, F), ref_mul(ref, F, F)
    f2, g2x2 = ref_sqn(ref, F, 1), ref_sqn(ref, G, 2)
    f2x2 = ref_sqn(ref, F, 2)
    H = {op: engine.debug_fe(op, F, G) for op in range(8)}
    for name, got, exp in (("fd_fe_mul", H[0][0], fg), ("fd_fe_sqn n=1", H[1][0], f2), ("fd_fe_sqn n=2", H[2][0], f2x2),
                           ("fd_fe_mul_ilp", H[3][0], fg), ("fd_fe_mul2 first", H[4][0], fg), ("fd_fe_mul2 second", H[4][1], gf),
                           ("fd_fe_chain3 first", H[5][0], fg), ("fd_fe_chain3 second", H[5][1], gf),
                           ("fd_fe_chain3 third", H[5][2], ff), ("fd_fe_sqn2 first", H[6][0], f2),
                           ("fd_fe_sqn2 second", H[6][1], g2x2), ("fd_o_mul (oct DSM half product)", H[7][0], fg)):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert len(bad) == 0, (what, name, len(bad), bad[:8], F[bad[:2]], G[bad[:2]], got[bad[:2]], exp[bad[:2]])


# limbs at the carry rounding boundaries (tests/test_fe_host.py::test_carry_edges_vs_oracle,
# which runs the host compile of the same functions)
EDGES = np.array([0, 1, -1, 1 << 24, -(1 << 24), (1 << 24) - 1, 1 << 25, -(1 << 25), (1 << 25) - 1,
                  (1 << 26) - 1, -(1 << 26)], np.int32)


def test_device_field_products_carry_edges_mixed(engine, ref):
    """every limb one of the carry-boundary values, mixed at random: 3,000 pairs"""
    rng = np.random.default_rng(9)
    F = rng.choice(EDGES, (3000, 10)).astype(np.int32)
    G = rng.choice(EDGES, (3000, 10)).astype(np.int32)
    check_all_ops(engine, ref, F, G, "mixed edges")


def test_device_field_products_carry_edges_one_hot(engine, ref):
    """each edge value in each limb position, the other limbs zero: against itself (a
    single column product, its carry and the 19-fold wrap alone) and against a dense
    random operand, either way round"""
    rng = np.random.default_rng(10)
    hot = np.zeros((len(EDGES) * 10, 10), np.int32)
    for a, v in enumerate(EDGES):
        for k in range(10):
            hot[10 * a + k, k] = v
    assert len(hot) == 110 and len({tuple(r) for r in hot.tolist()}) == 101      # the ten all-zero rows of edge 0 are one
    dense = rand_fe(rng, len(hot), 26)
    check_all_ops(engine, ref, hot, hot, "one-hot x itself")
    check_all_ops(engine, ref, hot, dense, "one-hot x dense")
    check_all_ops(engine, ref, dense, hot, "dense x one-hot")
    # every one-hot against every other position of the same value: all 100 column pairs of each edge
    F = np.repeat(hot, 10, axis=0)
    G = np.concatenate([hot[10 * a:10 * a + 10] for a in range(len(EDGES)) for _ in range(10)])
    check_all_ops(engine, ref, F, G, "one-hot x one-hot")


def test_device_field_products_args(engine):
    import firedancer_amd as fa
    with pytest.raises(fa.EngineError):
        engine.debug_fe(8, np.zeros((1, 10), np.int32), np.zeros((1, 10), np.int32))
    assert engine.debug_fe(0, np.zeros((0, 10), np.int32), np.zeros((0, 10), np.int32)).shape == (3, 0, 10)
