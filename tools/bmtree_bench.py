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
    a = ap.parse_args()
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

    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
