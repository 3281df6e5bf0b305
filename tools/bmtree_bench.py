#!/usr/bin/env python3
"""Merkle roots on one MI355X beside fd_bmtree_roots_batch on the host
threads of the same box.  One process, seeded inputs; every device root and
code is compared with the host's.

Lines (JSON, one per measurement, appended to --out):
  entry_mix   the PoH catch-up mix's entry structure (tools/poh_bench.py:
              --slots slots x 64 ticks x 0..32 transaction entries), each
              transaction entry a bmtree32 tree over a seeded 1..64 signatures
              of 64 bytes: device-resident (HIP events around the call),
              packed (staging and PCIe both ways) and the host
  one_tree    one bmtree32 tree of 1,048,576 64-byte leaves
  shred_like  4,096 bmtree20 trees of 64..134 leaves of 1,203 bytes
  crossover   prefixes of the entry mix (1, 2, 4, ... slots): packed device
              call against host
  end_to_end  Engine.poh_verify_entries against host roots followed by
              Engine.poh_verify on the same bytes, alternating pairs

With --proofs only the inclusion proof lines are measured, on the shred-like
load (results to profiles/r16_bmtree_proofs.jsonl unless --out is given):
  proofs_emit      fd_bmtree_gpu_proofs_dev against fd_bmtree_gpu_roots_dev on
                   the same resident inputs, --pairs alternating pairs (HIP
                   events), the packed emit, and fd_bmtree_proofs_batch on the
                   host; `extra_ms` is emit less roots-only, `row_bytes` the
                   N D W bytes of proof rows, `row_gbps` their rate over the
                   extra time
  proofs_verify    every leaf's proof walked (strict, EXPECT at its tree's
                   root): fd_bmtree_gpu_from_proofs_dev, _packed and
                   fd_bmtree_from_proofs_batch on the host
  proofs_crossover prefixes of the proofs: packed device call against host
Every device byte and code is compared with the host batch's.

Every record of a tree load carries `merge_passes`: the 64-lane compression
passes its merge launches issue, counted from the shapes
(fd_bmtree_gpu_merge_passes), beside `merge_passes_floor`, the merges' blocks
over 64.  Every rate is the median over --reps timed repetitions after
--warmup untimed ones; min and max are recorded beside it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import firedancer_amd as fa  # noqa: E402
from poh_bench import TICK, mix_entries, stats  # noqa: E402


def sig_leaves(cnt, seed):
    """64-byte leaves back to back for trees of cnt leaves: (leaves, blob)"""
    total = int(np.asarray(cnt, np.uint64).sum())
    leaves = np.zeros(total, fa.BMTREE_LEAF_DTYPE)
    leaves["off"] = np.arange(total, dtype=np.uint32) * 64
    leaves["sz"] = 64
    blob = np.random.default_rng(seed).integers(0, 256, 64 * total, dtype=np.uint8)
    return leaves, blob


def merges(cnt):
    """branch nodes of trees of cnt leaves"""
    total = 0
    for c in np.unique(cnt):
        k, c = int((cnt == c).sum()), int(c)
        while c > 1:
            c = (c + 1) // 2
            total += k * c
    return total


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r14_bmtree_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check of this tool)")
    ap.add_argument("--proofs", action="store_true", help="the inclusion proof lines only")
    a = ap.parse_args()
    if a.proofs and a.out == ap.get_default("out"):
        a.out = os.path.join(root, "profiles", "r16_bmtree_proofs.jsonl")
    import torch

    eng = fa.Engine(0, 1 << 12, 1 << 20, depth=1)
    dev = torch.device("cuda", 0)
    tstream = torch.cuda.Stream(dev)
    st = tstream.cuda_stream
    assert st
    lines = []

    def emit(kind, **kw):
        rec = {"tool": "bmtree_bench", "kind": kind, **kw}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def host(W, cnt, leaves, blob, leaf_max, reps=3):
        dts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r, c = fa.bmtree_roots_batch(W, cnt, leaves, blob, leaf_max, 0, a.host_threads)
            dts.append(time.perf_counter() - t0)
        return dts, r, c

    def packed(W, cnt, leaves, blob, leaf_max, reps, warm):
        dts = []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            r, c = eng.bmtree_roots(W, cnt, leaves, blob, leaf_max)
            dt = time.perf_counter() - t0
            if k >= warm:
                dts.append(dt)
        return dts, r, c

    def resident(W, cnt, leaves, blob, leaf_max, reps, warm):
        T, N = len(cnt), len(leaves)
        first = np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]).astype(np.uint32)
        d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
        d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
        d_blob = torch.from_numpy(blob).to(dev)
        d_roots = torch.zeros((T, 32), dtype=torch.uint8, device=dev)
        d_codes = torch.full((T,), 77, dtype=torch.int32, device=dev)
        d_work = torch.zeros(fa.bmtree_work_sz(T, N), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = []
        for k in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(tstream)
            eng.bmtree_roots_dev(W, T, d_first.data_ptr(), N, d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, leaf_max,
                                 d_roots.data_ptr(), 32, d_codes.data_ptr(), d_work.data_ptr(), st)
            e1.record(tstream)
            torch.cuda.synchronize()
            if k >= warm:
                ms.append(e0.elapsed_time(e1))
        return ms, d_roots.cpu().numpy(), d_codes.cpu().numpy()

    def load(kind, W, cnt, leaves, blob, leaf_max, **kw):
        cnt = np.asarray(cnt, np.uint32)
        hdt, hr, hc = host(W, cnt, leaves, blob, leaf_max)
        ms, rr, rc = resident(W, cnt, leaves, blob, leaf_max, a.reps, a.warmup)
        dts, pr, pc = packed(W, cnt, leaves, blob, leaf_max, a.reps, a.warmup)
        hmed, N = sorted(hdt)[len(hdt) // 2], len(leaves)
        m = merges(cnt)
        emit(kind, width=W, trees=len(cnt), leaves=N, blob_bytes=int(blob.nbytes), merges=m,
             merge_passes=fa.bmtree_merge_passes(W, cnt), merge_passes_floor=-(-m // 64) * (2 if W == 32 else 1),
             host_threads=a.host_threads, host_s=stats(hdt), resident_ms=stats(ms), packed_s=stats(dts),
             resident_leaves_per_s=stats([N / (x * 1e-3) for x in ms]), packed_leaves_per_s=stats([N / x for x in dts]),
             host_leaves_per_s=N / hmed, resident_over_host=hmed / (sorted(ms)[len(ms) // 2] * 1e-3),
             packed_over_host=hmed / sorted(dts)[len(dts) // 2],
             device_equals_host=bool((rc == hc).all() and (rr == hr).all() and (pc == hc).all() and (pr == hr).all()), **kw)

    def write_out():
        eng.close()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")

    def med(v):
        return sorted(v)[len(v) // 2]

    def proofs():
        """the shred-like load: emit beside roots-only, then every proof walked"""
        W, leaf_max = 20, 134
        rng = np.random.default_rng(7)
        cnt = rng.integers(64, 135, 64 if a.quick else 4096).astype(np.uint32)
        T, N = len(cnt), int(cnt.sum())
        leaves = np.zeros(N, fa.BMTREE_LEAF_DTYPE)
        leaves["off"] = np.arange(N, dtype=np.uint32) * 1203
        leaves["sz"] = 1203
        blob = rng.integers(0, 256, 1203 * N, dtype=np.uint8)
        stride = fa.bmtree_proof_stride(W, N, leaf_max)
        depth = np.array([(int(c) - 1).bit_length() for c in cnt], np.uint32)
        row_bytes = int((cnt.astype(np.uint64) * depth * W).sum())

        # host emit
        hdt = []
        for _ in range(3):
            t0 = time.perf_counter()
            hr, hc, hp = fa.bmtree_proofs_batch(W, cnt, leaves, blob, leaf_max, 0, a.host_threads)
            hdt.append(time.perf_counter() - t0)
        hrdt, hr0, hc0 = host(W, cnt, leaves, blob, leaf_max)
        assert (hc == 0).all() and (hr0 == hr).all()

        # resident: roots-only and emit, alternating
        first = np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]).astype(np.uint32)
        d_first = torch.from_numpy(first.view(np.int32).copy()).to(dev)
        d_leaves = torch.from_numpy(leaves.view(np.uint8).copy()).to(dev)
        d_blob = torch.from_numpy(blob).to(dev)
        d_roots = torch.zeros((T, 32), dtype=torch.uint8, device=dev)
        d_rows = torch.zeros((N, stride), dtype=torch.uint8, device=dev)
        d_codes = torch.full((T,), 77, dtype=torch.int32, device=dev)
        d_work = torch.zeros(fa.bmtree_work_sz(T, N), dtype=torch.uint8, device=dev)
        common = (W, T, d_first.data_ptr(), N, d_leaves.data_ptr(), d_blob.data_ptr(), blob.nbytes, leaf_max, d_roots.data_ptr(), 32)

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(tstream)
            call()
            e1.record(tstream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def roots_only():
            eng.bmtree_roots_dev(*common, d_codes.data_ptr(), d_work.data_ptr(), st)

        def with_rows():
            eng.bmtree_proofs_dev(*common, d_rows.data_ptr(), stride, d_codes.data_ptr(), d_work.data_ptr(), st)

        torch.cuda.synchronize()
        for _ in range(a.warmup):
            timed(roots_only)
            timed(with_rows)
        ms = {"roots": [], "emit": []}
        for p in range(a.pairs):
            for side in (("roots", "emit") if p % 2 == 0 else ("emit", "roots")):
                ms[side].append(timed(roots_only if side == "roots" else with_rows))
        same = bool((d_roots.cpu().numpy() == hr).all() and (d_codes.cpu().numpy() == hc).all() and (d_rows.cpu().numpy() == hp).all())

        # packed emit
        pdt = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            pr, pc, pp = eng.bmtree_proofs(W, cnt, leaves, blob, leaf_max)
            if k >= a.warmup:
                pdt.append(time.perf_counter() - t0)
        same = same and bool((pr == hr).all() and (pc == hc).all() and (pp == hp).all())
        extra = med(ms["emit"]) - med(ms["roots"])
        emit("proofs_emit", width=W, trees=T, leaves=N, blob_bytes=int(blob.nbytes), proof_stride=stride, row_bytes=row_bytes,
             pairs=a.pairs, host_threads=a.host_threads, resident_roots_ms=stats(ms["roots"]), resident_emit_ms=stats(ms["emit"]),
             resident_roots_all=ms["roots"], resident_emit_all=ms["emit"], extra_ms=extra,
             row_gbps=(row_bytes / (extra * 1e-3) / 1e9) if extra > 0 else None, packed_emit_s=stats(pdt),
             host_emit_s=stats(hdt), host_roots_s=stats(hrdt), resident_emit_over_host=med(hdt) / (med(ms["emit"]) * 1e-3),
             packed_emit_over_host=med(hdt) / med(pdt), device_equals_host=same)

        # verify: every leaf with its proof and its tree's root in one blob
        tree_of = np.repeat(np.arange(T, dtype=np.uint32), cnt)

        def walk_inputs(n):
            """the first n leaves, their proofs and their trees' roots as one blob with its descriptors"""
            t1 = int(tree_of[n - 1]) + 1
            rows_off, roots_off = 1203 * n, 1203 * n + n * stride
            vb = np.concatenate([blob[:1203 * n], hp[:n].reshape(-1), hr[:t1].reshape(-1)])
            d = np.zeros(n, fa.BMTREE_PROOF_DTYPE)
            d["leaf_off"] = leaves["off"][:n]
            d["leaf_sz"] = 1203
            d["proof_off"] = rows_off + np.arange(n, dtype=np.uint64) * stride
            d["idx"] = np.arange(n, dtype=np.uint32) - first[tree_of[:n]]
            d["leaf_cnt"] = cnt[tree_of[:n]]
            d["depth"] = depth[tree_of[:n]]
            d["expect_off"] = roots_off + 32 * tree_of[:n].astype(np.uint64)
            d["flags"] = fa.BMTREE_PROOF_EXPECT
            return d, vb

        desc, vblob = walk_inputs(N)
        del d_rows, d_work, d_blob
        torch.cuda.empty_cache()

        def host_walk(desc, vblob):
            dts = []
            for _ in range(3):
                t0 = time.perf_counter()
                r, c = fa.bmtree_from_proofs_batch(W, desc, vblob, 8, 0, a.host_threads)
                dts.append(time.perf_counter() - t0)
            return dts, r, c

        def packed_walk(desc, vblob, reps, warm):
            dts = []
            for k in range(warm + reps):
                t0 = time.perf_counter()
                r, c = eng.bmtree_from_proofs(W, desc, vblob, 8)
                if k >= warm:
                    dts.append(time.perf_counter() - t0)
            return dts, r, c

        wdt, wr, wc = host_walk(desc, vblob)
        assert (wc == 0).all() and (wr == hr[tree_of]).all()
        d_vblob = torch.from_numpy(vblob).to(dev)
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        d_wroots = torch.zeros((N, 32), dtype=torch.uint8, device=dev)
        d_wcodes = torch.full((N,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        vms = []
        for k in range(a.warmup + a.reps):
            t = timed(lambda: eng.bmtree_from_proofs_dev(W, N, d_desc.data_ptr(), d_vblob.data_ptr(), vblob.nbytes, 8,
                                                         d_wroots.data_ptr(), 32, d_wcodes.data_ptr(), st))
            if k >= a.warmup:
                vms.append(t)
        same = bool((d_wroots.cpu().numpy() == wr).all() and (d_wcodes.cpu().numpy() == wc).all())
        del d_vblob
        torch.cuda.empty_cache()
        vdt, vr, vc = packed_walk(desc, vblob, a.reps, a.warmup)
        same = same and bool((vr == wr).all() and (vc == wc).all())
        emit("proofs_verify", width=W, proofs=N, blob_bytes=int(vblob.nbytes), host_threads=a.host_threads, resident_ms=stats(vms),
             packed_s=stats(vdt), host_s=stats(wdt), resident_proofs_per_s=N / (med(vms) * 1e-3), packed_proofs_per_s=N / med(vdt),
             host_proofs_per_s=N / med(wdt), resident_over_host=med(wdt) / (med(vms) * 1e-3), packed_over_host=med(wdt) / med(vdt),
             device_equals_host=same)

        # where the host wins: prefixes of the proofs, each with a blob of its own
        n = 16
        while n < N:
            dn, bn = walk_inputs(n)
            dts_h, r_h, c_h = host_walk(dn, bn)
            dts_d, r_d, c_d = packed_walk(dn, bn, 3, 1)
            emit("proofs_crossover", proofs=n, blob_bytes=int(bn.nbytes), host_s=med(dts_h), device_s=med(dts_d),
                 device_over_host=med(dts_h) / med(dts_d), host_threads=a.host_threads,
                 device_equals_host=bool((r_d == r_h).all() and (c_d == c_h).all() and (c_h == 0).all()))
            n *= 4

    if a.proofs:
        proofs()
        write_out()
        return

    # the entry mix: one tree per transaction entry
    slots, tick = (4, 1250) if a.quick else (a.slots, TICK)
    ent, slot_at = mix_entries(slots, seed=3, tick=tick)
    rng = np.random.default_rng(4)
    ecnt = np.where(ent["flags"] != 0, rng.integers(1, 65, len(ent)), 0).astype(np.uint32)
    eleaves, eblob = sig_leaves(ecnt, 5)
    tx = ecnt > 0
    load("entry_mix", 32, ecnt[tx], eleaves, eblob, 64, slots=slots)

    # one large tree
    n1 = 1 << 12 if a.quick else 1 << 20
    l1, b1 = sig_leaves([n1], 6)
    load("one_tree", 32, [n1], l1, b1, n1)

    # shred-like: bmtree20 over 1,203-byte leaves
    rng = np.random.default_rng(7)
    scnt = rng.integers(64, 135, 64 if a.quick else 4096).astype(np.uint32)
    total = int(scnt.sum())
    sl = np.zeros(total, fa.BMTREE_LEAF_DTYPE)
    sl["off"] = np.arange(total, dtype=np.uint32) * 1203
    sl["sz"] = 1203
    load("shred_like", 20, scnt, sl, rng.integers(0, 256, 1203 * total, dtype=np.uint8), 134)

    # where the host wins: prefixes of the entry mix
    first = np.concatenate([[0], np.cumsum(ecnt, dtype=np.uint64)]).astype(np.int64)
    k = 1
    while k <= slots:
        e1 = slot_at[k]
        c, lv, bl = ecnt[:e1][tx[:e1]], eleaves[:first[e1]], eblob[:64 * first[e1]]
        hdt, hr, hc = host(32, c, lv, bl, 64)
        dts, pr, pc = packed(32, c, lv, bl, 64, 3, 1)
        emit("crossover", slots=k, trees=len(c), leaves=len(lv), host_s=sorted(hdt)[1], device_s=sorted(dts)[1],
             device_over_host=sorted(hdt)[1] / sorted(dts)[1], host_threads=a.host_threads,
             device_equals_host=bool((pc == hc).all() and (pr == hr).all()))
        k *= 2

    # end to end: entries from leaves on the device against host roots then poh_verify
    hroots, hcodes = fa.bmtree_roots_batch(32, ecnt[tx], eleaves, eblob, 64, 0, a.host_threads)
    assert (hcodes == 0).all()
    ref = ent.copy()
    ref["mixin"][tx] = hroots
    _, states = fa.poh_verify_batch(ref, tick, states=True, nthreads=a.host_threads)
    ref["expect"] = states
    ent["expect"] = states
    ab = {"entries": [], "host_roots_then_verify": [], "verify_alone": []}
    same = True
    for p in range(a.pairs):
        for side in (("entries", "host_roots_then_verify") if p % 2 == 0 else ("host_roots_then_verify", "entries")):
            t0 = time.perf_counter()
            if side == "entries":
                c, s = eng.poh_verify_entries(ent, tick, ecnt, eleaves, eblob, 64, states=True)
            else:
                r, _ = fa.bmtree_roots_batch(32, ecnt[tx], eleaves, eblob, 64, 0, a.host_threads)
                e2 = ent.copy()
                e2["mixin"][tx] = r
                c, s = eng.poh_verify(e2, tick, states=True)
            ab[side].append(time.perf_counter() - t0)
            same = same and bool((c == 0).all() and (s == states).all())
        t0 = time.perf_counter()
        eng.poh_verify(ref, tick, states=True)
        ab["verify_alone"].append(time.perf_counter() - t0)
    emit("end_to_end", entries=len(ent), trees=int(tx.sum()), leaves=len(eleaves), pairs=a.pairs, host_threads=a.host_threads,
         entries_s=stats(ab["entries"]), host_roots_then_verify_s=stats(ab["host_roots_then_verify"]),
         verify_alone_s=stats(ab["verify_alone"]), entries_all=ab["entries"], host_roots_then_verify_all=ab["host_roots_then_verify"],
         device_equals_host=same)

    write_out()


if __name__ == "__main__":
    main()
