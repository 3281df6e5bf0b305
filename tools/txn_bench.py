#!/usr/bin/env python3
"""What whole-transaction verification costs on one MI355X beside the
per-signature path it wraps, on the same bytes, in one process.

C2 shape (bench.py's workload): 1232-byte legacy transactions of 1-2
signatures from corpus.solana_txns, 256 x 4,096 signatures a step.

Lines (JSON, one per measurement, appended to --out):
  corpus          the batch: transactions, signatures, payload bytes
  check           verify_txns_dev's statuses and codes against verify_dev on descriptors
                  the host made from the same bytes, and against the host's reduction
  ab              --pairs pairs, alternating in this process: --steps steps of verify_dev
                  on host-made descriptors against as many of verify_txns_dev (parse,
                  scan, expand, the same verify pipeline, reduce); signatures/s medians
                  and ranges, and the transaction path's cost as a share of the step.
                  Both legs order each launch after the work on the stream, as
                  verify_txns_dev must (its descriptors are made there); verify_dev with
                  inputs_ready (bench.py's setting, launch k's front end over launch k-1's
                  DSM) is a third leg, so the overlap given up is on record too
  txn_kernels     HIP-event durations of the four new kernels over --reps launches
  packed          one leg with staging and PCIe at --packed-sigs signatures: verify_txns
                  (payloads and 8-byte entries in, 24-byte results out) against
                  verify_packed (host parse and expand not timed: descriptors ready)

--ring runs another comparison instead (lines appended to
profiles/r09_txn_ring.jsonl): the pinned ring at the C2 batch size, submit
on host-made descriptors against submit_txns on the same bytes, the same
engine, alternating pairs.  The C2 bytes are cut into batches of whole
transactions that claim at most 4,096 signatures.
  ring_corpus     the batches
  ring            one line per leg and per place the bytes lie (a registered region,
                  read in place; an ordinary array, staged): closed loop at --window
                  in flight (signatures/s) and a lone batch's round trip (p50, p99),
                  median and range over the pairs
  ring_check      the last pass's statuses and codes against the descriptor leg's codes
                  and their fold (the first nonzero code of each transaction)
  ring_kernels    HIP-event durations of fd_k_txn_ring_front and fd_k_txn_ring_reduce, in a
                  run of their own
  claims_cost     host ns per transaction of fd_ed25519_gpu_txn_claims on a warm and on a
                  cold blob
"""
import argparse
import collections
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import firedancer_amd as fa  # noqa: E402
from firedancer_amd import corpus  # noqa: E402

MTU = corpus.TXN_MTU


def stats(v):
    r = sorted(v)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1], "reps": len(r)}


def ring_batches(base, max_claim):
    """the C2 bytes cut into batches of whole transactions claiming at most max_claim
    signatures -> [(first transaction, transactions, first signature, signatures)]"""
    ntx = (len(base.blob) - 64) // MTU
    cnt = np.bincount((base.desc["sig_off"] // MTU).astype(np.int64), minlength=ntx)
    assert np.array_equal(cnt, base.blob[:ntx * MTU:MTU])          # the first payload byte is the claim
    end = np.cumsum(cnt)
    first = end - cnt
    out, a = [], 0
    while a < ntx:
        b = int(np.searchsorted(end, first[a] + max_claim, side="right"))     # transactions that end inside the budget
        out.append((a, b - a, int(first[a]), int(end[b - 1] - first[a])))
        a = b
    return out


def ring_main(a, root):
    import torch  # noqa: F401  (one HIP runtime, firedancer_amd._share_hip_runtime)
    L = fa.lib()
    BS = 4096
    t0 = time.time()
    base = corpus.solana_txns(a.unique or 64 * BS, seed=1000, nthreads=min(16, os.cpu_count() or 8))
    gen_s = time.time() - t0
    batches = [b for b in ring_batches(base, BS) if b[3] > BS - 2]   # whole batches only (the last one is short)
    nb = len(batches)
    assert nb >= 4
    span = max(n * MTU for _, n, _, _ in batches)
    lines = []

    def emit(kind, **kw):
        rec = {"tool": "txn_bench", "kind": kind, "kernels_id": fa.kernels_id(), **kw}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    emit("ring_corpus", batches=nb, txns_per_batch=stats([n for _, n, _, _ in batches]), sigs_per_batch=stats([k for _, _, _, k in batches]),
         blob_bytes_per_batch=span, unique_sigs=len(base), gen_s=gen_s, depth=a.depth, window=a.window)
    # per batch: the span of the blob, entries and descriptors relative to it
    blobs, ents, descs = [], [], []
    for ta, tn, sa, sn in batches:
        blobs.append(base.blob[ta * MTU:(ta + tn) * MTU])
        e = np.zeros(tn, fa.TXN_DTYPE)
        e["off"] = np.arange(tn, dtype=np.uint64) * MTU
        e["sz"] = MTU
        ents.append(e)
        d = base.desc[sa:sa + sn].copy()
        for f in ("sig_off", "pub_off", "msg_off"):
            d[f] -= ta * MTU
        descs.append(d)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    out_codes = [np.zeros(BS, np.int32) for _ in range(nb)]
    out_tcodes = [np.zeros(BS, np.int32) for _ in range(nb)]
    out_res = [np.zeros(len(e), fa.TXN_RESULT_DTYPE) for e in ents]

    for where in ("registered", "staged"):
        eng = fa.Engine(0, max_sigs=BS, max_blob=span + 64, depth=a.depth)
        eng.txns_reserve(max(len(e) for e in ents))
        if where == "registered":
            eng.register(base.blob)
        h = eng._h
        ticket = ctypes.c_ulong(0)
        tref = ctypes.byref(ticket)
        d_args = [(len(descs[i]), ptr(blobs[i]), blobs[i].nbytes, ptr(descs[i])) for i in range(nb)]
        t_args = [(len(ents[i]), ptr(blobs[i]), blobs[i].nbytes, ptr(ents[i])) for i in range(nb)]
        d_out = [ptr(o) for o in out_codes]
        t_out = [(ptr(r), ptr(c)) for r, c in zip(out_res, out_tcodes)]

        def sub_d(i):
            if L.fd_ed25519_gpu_submit(h, *d_args[i], tref):
                raise fa.EngineError("submit: " + fa.last_error())
            return ticket.value

        def sub_t(i):
            if L.fd_ed25519_gpu_submit_txns(h, *t_args[i], tref):
                raise fa.EngineError("submit_txns: " + fa.last_error())
            return ticket.value

        def poll_d(k, i):
            if L.fd_ed25519_gpu_poll(h, k, d_out[i], 1) != 1:
                raise fa.EngineError("poll: " + fa.last_error())

        def poll_t(k, i):
            if L.fd_ed25519_gpu_poll_txns(h, k, t_out[i][0], t_out[i][1], 1) != 1:
                raise fa.EngineError("poll_txns: " + fa.last_error())

        def closed(sub, poll, n, window):
            fl = collections.deque()
            i = 0
            t = time.perf_counter()
            for done in range(n):
                while len(fl) < window and i < n:
                    fl.append((sub(i % nb), i % nb))
                    i += 1
                poll(*fl.popleft())
            return time.perf_counter() - t

        def lone(sub, poll, n):
            dt = []
            for j in range(n):
                t = time.perf_counter()
                poll(sub(j % nb), j % nb)
                dt.append(time.perf_counter() - t)
            dt.sort()
            return 1e3 * dt[len(dt) // 2], 1e3 * dt[min(len(dt) - 1, int(0.99 * len(dt)))]

        legs = {"submit": (sub_d, poll_d, [len(d) for d in descs]), "submit_txns": (sub_t, poll_t, [len(d) for d in descs])}
        for sub, poll, _ in legs.values():                    # warm both
            closed(sub, poll, 2 * nb, a.window)
        got = {k: {"rate": [], "p50": [], "p99": []} for k in legs}
        for p in range(a.pairs):
            order = list(legs) if p % 2 == 0 else list(legs)[::-1]
            for name in order:
                sub, poll, sigs = legs[name]
                n = a.ring_batches
                wall = closed(sub, poll, n, a.window)
                got[name]["rate"].append(sum(sigs[i % nb] for i in range(n)) / wall)
                p50, p99 = lone(sub, poll, a.ring_lone)
                got[name]["p50"].append(p50)
                got[name]["p99"].append(p99)
        for name in legs:
            g = got[name]
            emit("ring", leg=name, where=where, pairs=a.pairs, batches_per_run=a.ring_batches, lone_batches_per_run=a.ring_lone,
                 window=a.window, depth=a.depth, closed_loop_sigs_per_s=stats(g["rate"]), lone_p50_ms=stats(g["p50"]),
                 lone_p99_ms=stats(g["p99"]), all=g)
        d_r, t_r = got["submit"], got["submit_txns"]
        emit("ring_verdict", where=where,
             txn_rate_inside_desc_range=bool(min(d_r["rate"]) <= stats(t_r["rate"])["median"] <= max(d_r["rate"])),
             txn_p50_inside_desc_range=bool(min(d_r["p50"]) <= stats(t_r["p50"])["median"] <= max(d_r["p50"])),
             rate_ratio_of_medians=stats(t_r["rate"])["median"] / stats(d_r["rate"])["median"],
             p50_diff_of_medians_ms=stats(t_r["p50"])["median"] - stats(d_r["p50"])["median"])
        # the last pass: every batch once through both legs, everything compared
        ok_status = ok_codes = ok_cnt = True
        rej = 0
        for i in range(nb):
            poll_d(sub_d(i), i)
            poll_t(sub_t(i), i)
            n_sig = len(descs[i])
            codes, res = out_codes[i][:n_sig], out_res[i]
            cnt = blobs[i][::MTU].astype(np.int64)
            first = np.cumsum(cnt) - cnt
            red = np.zeros(len(cnt), np.int32)
            for j in np.nonzero(codes)[0][::-1]:
                red[np.searchsorted(first, j, side="right") - 1] = codes[j]
            ok_status &= bool(np.array_equal(res["status"], red))
            ok_codes &= bool(np.array_equal(out_tcodes[i][:n_sig], codes))
            ok_cnt &= bool(np.array_equal(res["sig_cnt"], cnt) and np.array_equal(res["sig_base"], first))
            rej += int((codes != 0).sum())
        emit("ring_check", where=where, batches=nb, statuses_equal_fold_of_descriptor_codes=ok_status, codes_equal=ok_codes,
             sig_cnt_and_sig_base_equal=ok_cnt, rejected_signatures=rej)
        # the two ring kernels, HIP events, a run of their own
        ms = np.array([eng.txn_ring_timed(blobs[j % nb], ents[j % nb])[1] for j in range(a.reps + 1)][1:], np.float64)
        emit("ring_kernels", where=where, reps=a.reps,
             **{k: {"median_ms": float(np.median(ms[:, j])), "min_ms": float(ms[:, j].min()), "max_ms": float(ms[:, j].max())}
                for j, k in enumerate(fa.Engine.TXN_RING_KERNELS)})
        eng.close()

    # the host routine: ns per transaction, warm (the same batch again) and cold (512 MiB
    # walked through the caches before each call)
    bases = np.zeros(max(len(e) for e in ents) + 1, np.uint32)
    claims = lambda i: L.fd_ed25519_gpu_txn_claims(ptr(blobs[i]), blobs[i].nbytes, ptr(ents[i]), len(ents[i]), ptr(bases))  # noqa: E731
    warm, cold = [], []
    claims(0)
    for _ in range(a.reps):
        t = time.perf_counter()
        claims(0)
        warm.append(1e9 * (time.perf_counter() - t) / len(ents[0]))
    junk = np.ones(1 << 29, np.uint8)
    for r in range(a.reps):
        junk[::64] += 1
        i = 1 + r % (nb - 1)
        t = time.perf_counter()
        claims(i)
        cold.append(1e9 * (time.perf_counter() - t) / len(ents[i]))
    emit("claims_cost", txns_per_batch=len(ents[0]), warm_ns_per_txn=stats(warm), cold_ns_per_txn=stats(cold))

    os.makedirs(os.path.dirname(a.ring_out), exist_ok=True)
    with open(a.ring_out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "r08_txn_bench.jsonl"))
    ap.add_argument("--step-batches", type=int, default=256, help="4,096-signature batches a step")
    ap.add_argument("--unique", type=int, default=0, help="distinct signatures generated (0: a whole step's); the step tiles them")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed leg of a pair")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--packed-sigs", type=int, default=262144)
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check of this tool)")
    ap.add_argument("--ring", action="store_true", help="the pinned ring: submit on descriptors against submit_txns")
    ap.add_argument("--ring-out", default=os.path.join(root, "profiles", "r09_txn_ring.jsonl"))
    ap.add_argument("--depth", type=int, default=8, help="--ring: slots of the engine's ring")
    ap.add_argument("--window", type=int, default=8, help="--ring: batches in flight in the closed loop")
    ap.add_argument("--ring-batches", type=int, default=2000, help="--ring: batches per closed-loop run")
    ap.add_argument("--ring-lone", type=int, default=300, help="--ring: lone round trips per run")
    a = ap.parse_args()
    if a.quick:
        a.step_batches, a.packed_sigs, a.pairs = 4, 8192, 3
        a.ring_batches, a.ring_lone = 200, 50
        if a.ring and not a.unique:
            a.unique = 8 * 4096
    if a.ring:
        return ring_main(a, root)
    import torch

    n_step = a.step_batches * 4096
    t0 = time.time()
    base = corpus.solana_txns(a.unique or n_step, seed=1000, nthreads=min(16, os.cpu_count() or 8))
    gen_s = time.time() - t0
    reps_tile = -(-n_step // len(base))
    ntx1 = (len(base.blob) - 64) // MTU
    # the step: the unique transactions, tiled as bench.py tiles its descriptors (same bytes again)
    txns = np.zeros(ntx1 * reps_tile, fa.TXN_DTYPE)
    txns["off"] = np.tile(np.arange(ntx1, dtype=np.uint64) * MTU, reps_tile)
    txns["sz"] = MTU
    desc = np.tile(base.desc, reps_tile)
    n_sig = len(desc)                 # whole transactions: a little over n_step when tiled
    n_txn = len(txns)
    blob_sz = len(base.blob) - 64

    pk_sigs = min(a.packed_sigs, len(base))
    pk_txn = int(base.desc["sig_off"][pk_sigs - 1]) // MTU + 1
    pk_sigs = int((base.desc["sig_off"] // MTU < pk_txn).sum())
    eng = fa.Engine(0, max_sigs=max(n_sig, 1 << 16), max_blob=max(pk_txn * MTU + 64, 1 << 24), depth=2)
    eng.txns_reserve(max(n_txn, pk_txn))
    dev = torch.device("cuda", 0)
    tstream = torch.cuda.Stream(dev)
    st = tstream.cuda_stream
    assert st
    lines = []

    def emit(kind, **kw):
        rec = {"tool": "txn_bench", "kind": kind, "kernels_id": fa.kernels_id(), **kw}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    emit("corpus", txns=n_txn, sigs=n_sig, unique_sigs=len(base), payload_bytes=n_txn * MTU, distinct_payload_bytes=blob_sz, gen_s=gen_s)

    d_blob = torch.from_numpy(base.blob).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_txn = torch.from_numpy(txns.view(np.uint8).copy()).to(dev)
    d_out = torch.full((n_sig,), -1, dtype=torch.int32, device=dev)
    d_codes = torch.full((n_sig,), -1, dtype=torch.int32, device=dev)
    d_res = torch.zeros(3 * n_txn, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def leg_dev(ready):
        eng.verify_dev(n_sig, d_blob.data_ptr(), blob_sz, d_desc.data_ptr(), d_out.data_ptr(), st, inputs_ready=ready)

    def leg_txn(codes=True):
        eng.verify_txns_dev(n_txn, d_blob.data_ptr(), blob_sz, d_txn.data_ptr(), n_sig, d_res.data_ptr(),
                            d_codes.data_ptr() if codes else 0, 0, 0, st)

    def timed(fn, steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        tstream.synchronize()
        return n_sig * steps / (time.perf_counter() - t)

    # correctness first: the same verdicts as the per-signature path on host-made descriptors
    leg_dev(False)
    leg_txn()
    tstream.synchronize()
    res = d_res.cpu().numpy().view(fa.TXN_RESULT_DTYPE)
    host_codes = d_out.cpu().numpy()
    cnt = np.bincount((desc["sig_off"][:len(base)] // MTU).astype(np.int64), minlength=ntx1)
    # the host's reduction of the host-descriptor codes: the first nonzero code of each transaction
    first = np.cumsum(np.tile(cnt, reps_tile)) - np.tile(cnt, reps_tile)
    red = np.zeros(n_txn, np.int32)
    for i in np.nonzero(host_codes)[0][::-1]:
        red[np.searchsorted(first, i, side="right") - 1] = host_codes[i]
    # an all-valid corpus still holds the few signatures the reference itself rejects (ERR_MSG; bench.py valid_corpus_ok)
    rej = int((host_codes != 0).sum())
    emit("check", statuses_equal_host_reduction=bool(np.array_equal(res["status"], red)),
         codes_equal=bool(np.array_equal(d_codes.cpu().numpy(), host_codes)),
         sig_cnt_equal=bool(np.array_equal(res["sig_cnt"], np.tile(cnt, reps_tile))),
         sig_base_equal=bool(np.array_equal(res["sig_base"], first)),
         rejected_signatures=rej, rejected_transactions=int((res["status"] != 0).sum()),
         corpus_ok=bool(set(np.unique(host_codes).tolist()) <= {0, fa.ERR_MSG} and rej <= max(4, int(n_sig * 1e-5))), sig_total=n_sig)

    # alternating pairs
    rate = {"verify_dev": [], "verify_txns_dev": [], "verify_dev_inputs_ready": []}
    for fn in (lambda: leg_dev(False), leg_txn, lambda: leg_dev(True)):
        timed(fn, 2)                       # warm every leg once
    for p in range(a.pairs):
        order = [("verify_dev", lambda: leg_dev(False)), ("verify_txns_dev", leg_txn), ("verify_dev_inputs_ready", lambda: leg_dev(True))]
        if p % 2:
            order = order[1::-1] + order[2:]
        for name, fn in order:
            rate[name].append(timed(fn, a.steps))
    share = [1.0 - t / d for t, d in zip(rate["verify_txns_dev"], rate["verify_dev"])]
    step_ms = 1e3 * n_sig / stats(rate["verify_dev"])["median"]
    emit("ab", pairs=a.pairs, steps_per_leg=a.steps, sigs_per_step=n_sig, txns_per_step=n_txn,
         verify_dev_sigs_per_s=stats(rate["verify_dev"]), verify_txns_dev_sigs_per_s=stats(rate["verify_txns_dev"]),
         verify_dev_inputs_ready_sigs_per_s=stats(rate["verify_dev_inputs_ready"]),
         txn_share_of_step=stats(share), verify_dev_step_ms=step_ms,
         all={k: v for k, v in rate.items()})

    # the four new kernels, HIP events
    ms = np.array([eng.verify_txns_dev(n_txn, d_blob.data_ptr(), blob_sz, d_txn.data_ptr(), n_sig, d_res.data_ptr(), d_codes.data_ptr(),
                                       0, 0, st, timed=True) for _ in range(a.reps + 1)][1:], np.float64)
    med = np.median(ms, axis=0)
    emit("txn_kernels", reps=a.reps, **{k: {"median_ms": float(m), "min_ms": float(lo), "max_ms": float(hi)}
                                        for k, m, lo, hi in zip(fa.Engine.TXN_KERNELS, med, ms.min(axis=0), ms.max(axis=0))},
         sum_median_ms=float(med.sum()), share_of_verify_dev_step=float(med.sum() / step_ms))
    # with descriptors written too (stride 64 holds a C2 transaction's 30 bytes)
    d_tout = torch.zeros(64 * n_txn, dtype=torch.uint8, device=dev)
    ms = np.array([eng.verify_txns_dev(n_txn, d_blob.data_ptr(), blob_sz, d_txn.data_ptr(), n_sig, d_res.data_ptr(), d_codes.data_ptr(),
                                       d_tout.data_ptr(), 64, st, timed=True) for _ in range(a.reps + 1)][1:], np.float64)
    emit("txn_kernels_with_descriptors", reps=a.reps, stride=64, parse_median_ms=float(np.median(ms[:, 0])))

    # one packed leg with PCIe
    pk_blob = base.blob[:pk_txn * MTU + 64]
    pk_t, pk_d = txns[:pk_txn], base.desc[:pk_sigs]
    r_txn, r_pk = [], []
    for k in range(2 + a.reps):
        t0 = time.perf_counter()
        r = eng.verify_txns(pk_blob[:pk_txn * MTU], pk_t)
        t1 = time.perf_counter()
        c = eng.verify_packed(pk_blob, pk_d)
        t2 = time.perf_counter()
        if k >= 2:
            r_txn.append(pk_sigs / (t1 - t0))
            r_pk.append(pk_sigs / (t2 - t1))
    emit("packed", sigs=pk_sigs, txns=pk_txn, verify_txns_sigs_per_s=stats(r_txn), verify_packed_sigs_per_s=stats(r_pk),
         rejected_transactions=int((r["status"] != 0).sum()), rejected_signatures=int((c != 0).sum()),
         bytes_in_beside_payload={"verify_txns": 8 * pk_txn, "verify_packed": 16 * pk_sigs},
         bytes_out={"verify_txns": 24 * pk_txn, "verify_packed": 4 * pk_sigs})

    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
