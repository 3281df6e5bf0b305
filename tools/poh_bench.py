#!/usr/bin/env python3
"""Proof-of-History verification on one MI355X beside the host routine on the
same box.  One process, seeded inputs; every device code and state is
compared with fd_poh_verify_batch's (the full-chunk launch: a sample of its
lanes, the record says how many).

Lines (JSON, one per measurement, appended to --out):
  uniform      device-resident (Engine.poh_verify_dev, HIP events around the
               call), n = 2,048 hashes on 4,096, 65,536 and 262,144 lanes
  full_chunk   one launch at the default chunk: n = 16,384 on 131,072 lanes
  host         fd_poh_verify_batch on --host-threads threads over the mix
  mix          the catch-up mix through Engine.poh_verify (staging, PCIe both
               ways, the sort): --slots slots x 64 tick intervals of 12,500
               hashes, each interval cut at 0..32 uniformly chosen points into
               mixin entries (L - 1 appends, then the mixin) and then its tick
  sort_ab      the mix with the lanes sorted by n against the caller's order,
               alternating pairs
  crossover    prefixes of the mix (1, 2, 4, ... slots): device against host

Every rate is the median over --reps timed repetitions after --warmup untimed
ones; min and max are recorded beside it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import firedancer_amd as fa  # noqa: E402

TICK = 12500
TICKS_PER_SLOT = 64


def stats(v):
    r = sorted(v)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1], "reps": len(r)}


def uniform_entries(lanes, n, seed):
    rng = np.random.default_rng(seed)
    ent = np.zeros(lanes, fa.POH_ENTRY_DTYPE)
    ent["start"] = rng.integers(0, 256, (lanes, 32), dtype=np.uint8)
    ent["n"] = n
    return ent


def mix_entries(slots, seed, tick=TICK):
    """the catch-up mix; returns (entries, first entry of each slot)"""
    rng = np.random.default_rng(seed)
    ns, fl, slot_at = [], [], []
    for s in range(slots):
        slot_at.append(len(ns))
        for _ in range(TICKS_PER_SLOT):
            k = int(rng.integers(0, 33))
            cuts = np.sort(rng.choice(np.arange(1, tick), size=k, replace=False)) if k else np.zeros(0, np.int64)
            edges = np.concatenate([[0], cuts, [tick]])
            seg = np.diff(edges)
            ns.extend((seg[:-1] - 1).tolist())      # an entry with transactions: L - 1 appends, then the mixin
            fl.extend([fa.POH_MIXIN] * k)
            ns.append(int(seg[-1]))                 # the tick: appends only
            fl.append(0)
    slot_at.append(len(ns))
    ent = np.zeros(len(ns), fa.POH_ENTRY_DTYPE)
    ent["start"] = rng.integers(0, 256, (len(ns), 32), dtype=np.uint8)
    ent["mixin"] = rng.integers(0, 256, (len(ns), 32), dtype=np.uint8)
    ent["n"], ent["flags"] = ns, fl
    return ent, slot_at


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r13_poh_bench.jsonl"))
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
    tstream = torch.cuda.Stream(dev)        # events on a stream of our own bracket the launches queued on it
    st = tstream.cuda_stream
    assert st
    lines = []

    def emit(kind, **kw):
        rec = {"tool": "poh_bench", "kind": kind, "chunk": eng.poh_chunk, **kw}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def host(ent, n_max, threads=a.host_threads):
        t0 = time.perf_counter()
        codes, states = fa.poh_verify_batch(ent, n_max, states=True, nthreads=threads)
        return time.perf_counter() - t0, codes, states

    def dev_resident(ent, n_max, reps, warm):
        n = len(ent)
        d_ent = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
        d_out = torch.full((n,), 77, dtype=torch.int32, device=dev)
        d_st = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_work = torch.zeros(fa.poh_work_sz(n), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = []
        for k in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(tstream)
            eng.poh_verify_dev(n, d_ent.data_ptr(), n_max, d_out.data_ptr(), d_st.data_ptr(), d_work.data_ptr(), st)
            e1.record(tstream)
            torch.cuda.synchronize()
            if k >= warm:
                ms.append(e0.elapsed_time(e1))
        return ms, d_out.cpu().numpy(), d_st.cpu().numpy()

    # uniform load, device-resident
    n_u = 256 if a.quick else 2048
    for lanes in ((256, 1024) if a.quick else (4096, 65536, 262144)):
        ent = uniform_entries(lanes, n_u, seed=lanes)
        dt, _, hstates = host(ent, n_u)
        ent["expect"] = hstates
        ms, codes, states = dev_resident(ent, n_u, a.reps, a.warmup)
        emit("uniform", lanes=lanes, n=n_u, ms=stats(ms), hashes_per_s=stats([lanes * n_u / (m * 1e-3) for m in ms]),
             us_per_hash_per_lane=sorted(ms)[len(ms) // 2] * 1e3 / n_u, host_hashes_per_s=lanes * n_u / dt,
             host_threads=a.host_threads, device_equals_host=bool((codes == 0).all() and (states == hstates).all()))

    # one launch at the default chunk
    lanes, n_c = (1024, 1024) if a.quick else (131072, eng.poh_chunk)
    ent = uniform_entries(lanes, n_c, seed=7)
    ms, codes, states = dev_resident(ent, n_c, 3, 1)
    sample = np.random.default_rng(1).choice(lanes, 512, replace=False)
    _, _, hstates = host(ent[sample], n_c)
    emit("full_chunk", lanes=lanes, n=n_c, launch_ms=stats(ms), hashes_per_s=stats([lanes * n_c / (m * 1e-3) for m in ms]),
         lanes_checked=len(sample), device_equals_host=bool((states[sample] == hstates).all()))

    # the catch-up mix
    slots, tick = (4, 1250) if a.quick else (a.slots, TICK)
    ent, slot_at = mix_entries(slots, seed=3, tick=tick)
    hashes = int(ent["n"].sum()) + int((ent["flags"] != 0).sum())
    hdt = []
    for k in range(3):
        dt, hcodes, hstates = host(ent, tick)
        hdt.append(dt)
    ent["expect"] = hstates
    emit("host", entries=len(ent), slots=slots, hashes=hashes, threads=a.host_threads, s=stats(hdt),
         hashes_per_s=stats([hashes / t for t in hdt]))

    def packed(e, reps, warm):
        dts = []
        for k in range(warm + reps):
            t0 = time.perf_counter()
            codes, states = eng.poh_verify(e, tick, states=True)
            dt = time.perf_counter() - t0
            if k >= warm:
                dts.append(dt)
        return dts, codes, states

    dts, codes, states = packed(ent, a.reps, a.warmup)
    ok = bool((codes == 0).all() and (states == hstates).all())
    emit("mix", entries=len(ent), slots=slots, hashes=hashes, s=stats(dts), hashes_per_s=stats([hashes / t for t in dts]),
         entries_per_s=stats([len(ent) / t for t in dts]), device_over_host=sorted(hdt)[1] / sorted(dts)[len(dts) // 2],
         device_equals_host=ok)

    # sorted against caller-order lanes, alternating
    ab = {True: [], False: []}
    same = True
    for p in range(a.pairs):
        for srt in ((True, False) if p % 2 == 0 else (False, True)):
            eng.poh_debug_sort(srt)
            d, c, s = packed(ent, 1, 0)
            ab[srt].append(d[0])
            same = same and bool((c == 0).all() and (s == hstates).all())
    eng.poh_debug_sort(True)
    emit("sort_ab", entries=len(ent), pairs=a.pairs, sorted_s=stats(ab[True]), caller_order_s=stats(ab[False]),
         sorted_all=ab[True], caller_order_all=ab[False], device_equals_host=same)

    # where the host wins: prefixes of the mix
    k = 1
    while k <= slots:
        sub = ent[:slot_at[k]]
        sub_h = int(sub["n"].sum()) + int((sub["flags"] != 0).sum())
        h = sorted(host(sub, tick)[0] for _ in range(3))[1]
        d, c, s = packed(sub, 3, 1)
        emit("crossover", slots=k, entries=len(sub), hashes=sub_h, host_s=h, device_s=sorted(d)[1],
             device_over_host=h / sorted(d)[1], device_equals_host=bool((c == 0).all() and (s == hstates[:len(sub)]).all()))
        k *= 2

    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
