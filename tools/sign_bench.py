#!/usr/bin/env python3
"""Signing throughput on one MI355X beside the host signer on the same box.

Lines (JSON, one per measurement, appended to --out):
  sign_dev        device-resident signs/s at 2^18 and 2^20 signatures of 128-byte
                  messages (keys derived on the device), HIP events around each launch
  sign_packed     signs/s with staging and PCIe both ways, at 4,096 and 262,144
  public          public_from_seeds keys/s at 262,144
  host_sign       fd_ed25519_sign_batch on 16 threads, the same corpus, the same run
  inversion_ab    the point encodings' inversion, per lane against batched over a
                  wave, alternating in this process (pairs of device-resident launches)
  clock           the shader clock the verify pool ran at over the 2^18 signatures just
                  made (fd_ed25519_gpu_dsm_clock, as bench.py records it): the box's
                  clock under load, and every signature verified

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


def corpus(n, msg_sz, seed=1):
    """blob = per signature [seed 32 | message msg_sz], sign descriptors deriving the key"""
    rng = np.random.default_rng(seed)
    stride = 32 + msg_sz
    blob = rng.integers(0, 256, n * stride, dtype=np.uint8)
    d = np.zeros(n, fa.SIGN_DESC_DTYPE)
    d["seed_off"] = np.arange(n, dtype=np.uint64) * stride
    d["pub_off"] = fa.SIGN_DERIVE
    d["msg_off"] = d["seed_off"] + 32
    d["msg_sz"] = msg_sz
    seeds = blob.reshape(n, stride)[:, :32].copy()
    return blob, d, seeds


def stats(rates):
    r = sorted(rates)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1], "reps": len(r)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_sign_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--msg-sz", type=int, default=128)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--quick", action="store_true", help="small sizes (a functional check of this tool)")
    a = ap.parse_args()
    import torch

    big, mid, small = (1 << 14, 1 << 13, 1 << 10) if a.quick else (1 << 20, 1 << 18, 1 << 12)
    eng = fa.Engine(0, big, big * (32 + a.msg_sz) + 4096, depth=2)
    dev = torch.device("cuda", 0)
    # a stream of our own: the default stream's handle is 0, which the engine reads as "its own stream",
    # and events recorded on the default stream would not bracket the launch
    tstream = torch.cuda.Stream(dev)
    st = tstream.cuda_stream
    assert st
    L = fa.lib()
    default_inv = L.fd_ed25519_gpu_sign_set_batch_inv(0)
    L.fd_ed25519_gpu_sign_set_batch_inv(default_inv)
    lines = []

    def emit(kind, **kw):
        rec = {"tool": "sign_bench", "kind": kind, "msg_sz": a.msg_sz, "kernels_id": fa.kernels_id(),
               "batch_inv_default": default_inv, **kw}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def dev_time(n, d_blob, blob_sz, d_desc, d_sig, d_pub, d_codes, reps, warm):
        ms = []
        for k in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(tstream)
            eng.sign_dev(n, d_blob.data_ptr(), blob_sz, d_desc.data_ptr(), d_sig.data_ptr(), d_pub.data_ptr(), d_codes.data_ptr(), st)
            e1.record(tstream)
            torch.cuda.synchronize()
            if k >= warm:
                ms.append(e0.elapsed_time(e1))
        return ms

    blob, desc, seeds = corpus(big, a.msg_sz)
    stride = 32 + a.msg_sz
    d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).to(dev)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_sig = torch.zeros(64 * big, dtype=torch.uint8, device=dev)
    d_pub = torch.zeros(32 * big, dtype=torch.uint8, device=dev)
    d_codes = torch.zeros(big, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    # host signer, the yardstick: same corpus, same box, same run
    off = (np.arange(mid, dtype=np.uint64) * stride + 32)
    sz = np.full(mid, a.msg_sz, np.uint32)
    hpub, hsig = np.zeros((mid, 32), np.uint8), np.zeros((mid, 64), np.uint8)
    rates = []
    for k in range(3):
        t0 = time.perf_counter()
        L.fd_ed25519_sign_batch(mid, fa._p(seeds), fa._p(blob), fa._p(off), fa._p(sz), fa._p(hpub), fa._p(hsig), a.host_threads)
        rates.append(mid / (time.perf_counter() - t0))
    emit("host_sign", n=mid, threads=a.host_threads, signs_per_s=stats(rates))

    # device-resident
    for n in (mid, big):
        ms = dev_time(n, d_blob, n * stride, d_desc, d_sig, d_pub, d_codes, a.reps, a.warmup)
        emit("sign_dev", n=n, signs_per_s=stats([n / (m * 1e-3) for m in ms]), ms_median=sorted(ms)[len(ms) // 2])
    got = d_sig[:64 * mid].cpu().numpy().reshape(mid, 64)
    same = bool((got == hsig).all() and (d_pub[:32 * mid].cpu().numpy().reshape(mid, 32) == hpub).all())
    emit("check", n=mid, device_equals_host_signer=same)

    # the box's clock under load: the verify pool over the signatures just made
    vb = np.concatenate([blob[:mid * stride], np.zeros((-mid * stride) % 16, np.uint8)])
    base = len(vb)
    d_vblob = torch.cat([torch.from_numpy(vb).to(dev), d_sig[:64 * mid], d_pub[:32 * mid], torch.zeros(64, dtype=torch.uint8, device=dev)])
    vdesc = np.zeros(mid, fa.DESC_DTYPE)
    vdesc["sig_off"] = base + 64 * np.arange(mid)
    vdesc["pub_off"] = base + 64 * mid + 32 * np.arange(mid)
    vdesc["msg_off"], vdesc["msg_sz"] = off, a.msg_sz
    d_vdesc = torch.from_numpy(vdesc.view(np.uint8).copy()).to(dev)
    d_vout = torch.full((mid,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.dsm_clock(clear=True)
    for _ in range(3):
        eng.verify_dev(mid, d_vblob.data_ptr(), base + 96 * mid, d_vdesc.data_ptr(), d_vout.data_ptr(), st)
    torch.cuda.synchronize()
    clk = eng.dsm_clock()
    emit("clock", n=mid, all_verified=bool((d_vout.cpu().numpy() == 0).all()),
         pool_effective_clock_ghz=clk["pool"]["ghz"], pool_waves=clk["pool"]["waves"], quad_effective_clock_ghz=clk["quad"]["ghz"])

    # inversion A/B, alternating in this process
    ab = {0: [], 1: []}
    for p in range(a.pairs):
        for inv in ((0, 1) if p % 2 == 0 else (1, 0)):
            L.fd_ed25519_gpu_sign_set_batch_inv(inv)
            ms = dev_time(mid, d_blob, mid * stride, d_desc, d_sig, d_pub, d_codes, 1, 1 if p == 0 else 0)
            ab[inv].append(mid / (ms[0] * 1e-3))
    L.fd_ed25519_gpu_sign_set_batch_inv(default_inv)
    emit("inversion_ab", n=mid, pairs=a.pairs, per_lane_signs_per_s=stats(ab[0]), wave_batched_signs_per_s=stats(ab[1]),
         per_lane_all=ab[0], wave_batched_all=ab[1])

    # packed: staging, H2D, kernels, D2H
    for n in (small, mid):
        b, d = blob[:n * stride], desc[:n]
        rates = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            sig, pub, codes = eng.sign_packed(b, d)
            dt = time.perf_counter() - t0
            if k >= a.warmup:
                rates.append(n / dt)
        emit("sign_packed", n=n, signs_per_s=stats(rates), equals_host_signer=bool((sig[:min(n, mid)] == hsig[:min(n, mid)]).all()))

    rates = []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        pub = eng.public_from_seeds(seeds[:mid])
        dt = time.perf_counter() - t0
        if k >= a.warmup:
            rates.append(mid / dt)
    emit("public", n=mid, keys_per_s=stats(rates), equals_host_signer=bool((pub == hpub).all()))

    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
