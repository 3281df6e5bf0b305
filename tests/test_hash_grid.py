"""The hash-path grid (tests/hash_grid.py) checked on the CPU: these are
conditions on the inputs of tests/test_gpu_hash_paths.py, met by the reference
build alone (oracle/_ref/libfdref.so) -- no device code runs here."""
import numpy as np
import pytest

import firedancer_amd as fa
import hash_grid as hg


@pytest.fixture(scope="module")
def g(ref):
    return hg.grid(ref)


def test_counts(g):
    k = g.rows.kind
    assert (k == hg.GRID).sum() == 6432 and (k == hg.GIANT).sum() == 24 and (k >= hg.DEAD_SIG).sum() == 400
    for d in (hg.DEAD_SIG, hg.DEAD_Q1, hg.DEAD_PAST, hg.DEAD_WRAP):
        assert (k == d).sum() == 100
    assert len(g.ragged) == len(g.sorted) == 6856
    f = g.flip_rows
    assert len(f.sources) == 64 + 24 and len(set(f.sources)) == 88
    assert set(f.origin.tolist()) == set(int(x) for x in f.sources)
    # a shorter copy of every source row, and every position flip_positions names
    assert (f.what == -1).sum() == 88
    for i in f.sources:
        assert sorted(f.what[(f.origin == i) & (f.what >= 0)].tolist()) == hg.flip_positions(int(g.rows.sz[i]), int(g.rows.align[i]))
    assert len(g.flips) <= 8192 and g.flips.blob.nbytes <= (1 << 23)
    assert max(g.ragged.blob.nbytes, g.sorted.blob.nbytes) <= (1 << 23)


def test_every_residue_at_every_alignment(g):
    """all 128 x 16 (residue, alignment) pairs at each of the two prefixes, at 1-4 blocks"""
    r = g.rows
    grid = r.kind == hg.GRID
    for pre in (64, 0):
        pairs = set(zip(((pre + r.sz[grid]) % 128).tolist(), r.align[grid].tolist()))
        assert len(pairs) == 128 * 16, pre
        nb = hg.nblk(r.sz[grid], pre)
        assert set(nb.tolist()) == {1, 2, 3, 4}
        # every residue on a final block that is not the first, too
        assert len(set(((pre + r.sz[grid][nb > 1]) % 128).tolist())) == 128
    gi = r.kind == hg.GIANT
    assert sorted(set(r.sz[gi].tolist())) == sorted(hg.GIANT_LENS) and set(r.align[gi].tolist()) == set(hg.GIANT_ALIGNS)


@pytest.mark.parametrize("name", ["ragged", "sorted", "flips"])
def test_layout(g, name):
    p = getattr(g, name)
    d = p.desc
    so, po, mo = (d[k].astype(np.int64) for k in ("sig_off", "pub_off", "msg_off"))
    inb = p.kind <= hg.DEAD_Q1
    assert ((mo % 16)[inb] == p.align[inb]).all()
    assert ((so % 16) != (po % 16)).all() and ((so % 16)[inb] != (mo % 16)[inb]).all() and ((po % 16)[inb] != (mo % 16)[inb]).all()
    # nothing overlaps and nothing touches: a byte of noise at least between any two pieces
    iv = sorted([(int(a), int(a) + 64) for a in so] + [(int(a), int(a) + 32) for a in po]
                + [(int(a), int(a) + int(s)) for a, s in zip(mo[inb], d["msg_sz"][inb])])
    assert iv[0][0] >= 1 and all(x[1] < y[0] for x, y in zip(iv, iv[1:]))
    # the last live row's message ends the blob
    last = np.nonzero(p.kind <= hg.GIANT)[0][-1]
    assert int(mo[last]) + int(d["msg_sz"][last]) == p.blob.nbytes and d["msg_sz"][last] >= 16
    assert iv[-1][1] == p.blob.nbytes
    # the bytes are what the rows say
    rows = g.flip_rows if name == "flips" else g.rows
    for j in list(range(0, len(p), 97)) + [int(last)]:
        i = int(p.row[j])
        assert p.blob[so[j]:so[j] + 64].tobytes() == rows.sig[i].tobytes() and p.blob[po[j]:po[j] + 32].tobytes() == rows.pub[i].tobytes()
        if inb[j]:
            assert p.blob[mo[j]:mo[j] + int(d["msg_sz"][j])].tobytes() == rows.msg(i)
    # the descriptors that leave the blob
    past, wrap = p.kind == hg.DEAD_PAST, p.kind == hg.DEAD_WRAP
    assert (mo[past] + d["msg_sz"][past] == p.blob.nbytes + 1).all()
    assert (((mo[wrap] + d["msg_sz"][wrap]) & 0xffffffff) <= p.blob.nbytes).all() and (mo[wrap] + d["msg_sz"][wrap] > 2**32).all()


def test_orders(g):
    """every wave of the ragged order holds at least three block counts, at least 90 %
    of its waves a dead row (and a giant lane sits beside one-block lanes somewhere);
    the sorted order is by length"""
    p = g.ragged
    n = len(p)
    nb = np.where(p.kind <= hg.GIANT, hg.nblk(p.sz), 0)
    waves = [slice(w, min(w + 64, n)) for w in range(0, n, 64)]
    assert all(len(set(nb[w][nb[w] > 0].tolist())) >= 3 for w in waves)
    assert sum(bool((nb[w] == 0).any()) for w in waves) >= 0.9 * len(waves)
    assert any((nb[w] >= 30).any() and (nb[w] == 1).any() and (nb[w] == 0).any() for w in waves)
    assert sorted(p.row.tolist()) == list(range(len(g.rows)))
    s = g.sorted
    ls = s.sz[s.kind <= hg.GIANT]
    assert (np.diff(ls) >= 0).all() and sorted(s.row.tolist()) == list(range(len(g.rows)))
    # dead rows spread evenly: never 64 rows without one
    for q in (p, s):
        dead = np.nonzero(q.kind >= hg.DEAD_SIG)[0]
        assert np.diff(dead).max() <= 18 and dead[0] == 0 and n - dead[-1] <= 18


def test_reference_codes(g):
    """the reference accepts every valid row and gives ERR_MSG on every flip row; the
    dead rows get ERR_SIG, the early accept and (the engine's own) ERR_ARG"""
    for p in (g.ragged, g.sorted):
        assert (p.exp[p.kind <= hg.GIANT] == fa.SUCCESS).all(), np.nonzero((p.exp != 0) & (p.kind <= hg.GIANT))[0][:8]
        assert (p.exp[p.kind == hg.DEAD_SIG] == fa.ERR_SIG).all()
        assert (p.exp[p.kind == hg.DEAD_Q1] == fa.SUCCESS).all()
        assert (p.exp[p.kind >= hg.DEAD_PAST] == fa.ERR_ARG).all()
    assert (g.ragged.exp[np.argsort(g.ragged.row)] == g.sorted.exp[np.argsort(g.sorted.row)]).all()
    bad = np.nonzero(g.flips.exp != fa.ERR_MSG)[0]
    assert len(bad) == 0, [(int(g.flip_rows.origin[i]), int(g.flip_rows.what[i]), int(g.flips.exp[i])) for i in bad[:8]]


def test_digest_helper(g):
    """hash_grid.digests is hashlib over R || A || M of the packed bytes; spot-checked
    against the rows' own store"""
    import hashlib
    p = g.ragged
    dig = hg.digests(p)
    for j in range(0, len(p), 211):
        i = int(p.row[j])
        if p.kind[j] <= hg.GIANT:
            want = hashlib.sha512(g.rows.sig[i, :32].tobytes() + g.rows.pub[i].tobytes() + g.rows.msg(i)).digest()
            assert dig[j].tobytes() == want
        else:
            assert not dig[j].any()
