#!/usr/bin/env python3
"""The SHA-512 batch backend on one MI355X: the long path in absolute terms,
the short path against another checkout, ping-pong against one buffer.

Every measurement is a process of its own (`leg`), so that two libraries are
compared by alternating fresh processes on one box; `run` starts the legs
one after another, stops at the first that fails, and appends one JSON line
per measurement to --out:

  long_abs      fini over N messages of SZ bytes on the default engine, GB/s
                with packing and PCIe; the reference's fd_sha512 on 16 host
                threads over the same bytes in the same process beside it
  short_ab      fini over 262,144 messages of 1 KB: this tree against --parent
                (another checkout of the repository, built), alternating pairs
  pingpong_ab   the long path with FD_SHA_LONG_PINGPONG 1 (this tree's library)
                against 0 (--pp0-lib, a build with -DFD_SHA_LONG_PINGPONG=0),
                alternating pairs, at 4,096 x 256 KB and 1 x 64 MB
  bench_ab      python bench.py --gpus 1 --steps 20 --warmup 5 in this tree and
                in --parent, alternating

A leg times fd_sha512_gpu_batch_fini alone (the queue is filled before the
clock starts), checks digests against hashlib, and with --clock reads the
shader clock the verify pool ran at on the same box right after
(fd_ed25519_gpu_dsm_clock, as bench.py records it)."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    r = sorted(v)
    return {"median": r[len(r) // 2], "min": r[0], "max": r[-1], "reps": len(r)}


def find_key(j, key):
    """the first value of key anywhere in a JSON tree"""
    if isinstance(j, dict):
        if key in j:
            return j[key]
        j = list(j.values())
    if isinstance(j, list):
        for v in j:
            r = find_key(v, key)
            if r is not None:
                return r
    return None


def leg(a):
    import numpy as np
    tree = os.path.abspath(a.tree or ROOT)
    sys.path.insert(0, tree)
    import firedancer_amd as fa
    L = fa.lib()
    n, sz = a.n, a.sz
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, n * sz, dtype=np.uint8)
    out = np.zeros(n * 64, np.uint8)
    eng = fa.Engine()
    b = L.fd_sha512_gpu_batch_new(eng._h, 0)
    assert b
    dp, op = data.ctypes.data, out.ctypes.data
    secs = []
    for k in range(a.warmup + a.reps):
        out[:] = 0
        L.fd_sha512_gpu_batch_init(b)
        for i in range(n):
            L.fd_sha512_gpu_batch_add(b, dp + i * sz, sz, op + 64 * i)
        t0 = time.perf_counter()
        r = L.fd_sha512_gpu_batch_fini(b)
        dt = time.perf_counter() - t0
        assert r == b, fa.last_error()
        if k >= a.warmup:
            secs.append(dt)
    for i in sorted({0, n // 2, n - 1}):
        assert out[64 * i:64 * i + 64].tobytes() == hashlib.sha512(data[i * sz:(i + 1) * sz].tobytes()).digest(), i
    L.fd_sha512_gpu_batch_delete(b)
    rec = {"n": n, "sz": sz, "seconds": secs, "gb_per_s": [n * sz / s / 1e9 for s in secs], "tree": tree,
           "lib": os.path.abspath(fa.LIB_PATH), "kernels_id": fa.kernels_id()}
    if a.ref_threads:
        R = ctypes.CDLL(os.path.join(tree, "oracle", "_ref", "libfdref.so"))
        R.ref_sha512.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_void_p]
        rout = np.zeros(n * 64, np.uint8)
        rp = rout.ctypes.data

        def work(t):
            for i in range(t, n, a.ref_threads):
                R.ref_sha512(dp + i * sz, sz, rp + 64 * i)
        rs = []
        for _ in range(3):
            th = [threading.Thread(target=work, args=(t,)) for t in range(a.ref_threads)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            rs.append(time.perf_counter() - t0)
        assert (rout == out).all()
        rec.update(ref_threads=a.ref_threads, ref_seconds=rs, ref_gb_per_s=[n * sz / s / 1e9 for s in rs])
    eng.close()
    if a.clock:
        try:
            from firedancer_amd import corpus
            vb = corpus.simple(1 << 18, 64, 3, 16)
            ceng = fa.Engine(0, 1 << 18, 1 << 26, depth=1)      # the pooled DSM takes batches of 2^18 and up
            ceng.dsm_clock(clear=True)
            for _ in range(2):
                codes = ceng.verify_packed(vb.blob, vb.desc)
            clk = ceng.dsm_clock()
            ceng.close()
            rec.update(pool_effective_clock_ghz=clk["pool"]["ghz"], pool_waves=clk["pool"]["waves"], all_verified=bool((codes == 0).all()))
        except Exception as e:      # the clock is a rider: the measurement stands without it
            rec.update(pool_effective_clock_ghz=None, clock_error=repr(e))
    print("SHA_BENCH " + json.dumps(rec), flush=True)


def child(args, env=None, cwd=None, limit=300):
    """one measurement in a fresh process; a failure, a fault or a time limit ends the whole run"""
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run(args, capture_output=True, text=True, timeout=limit, env=e, cwd=cwd)
    if r.returncode:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"sha_bench: {' '.join(args)} ended with {r.returncode}: stopping")
    return r.stdout


def run_leg(n, sz, reps, warmup, tree=None, lib=None, ref_threads=0, clock=False, limit=300):
    args = [sys.executable, os.path.abspath(__file__), "leg", "--n", str(n), "--sz", str(sz), "--reps", str(reps), "--warmup", str(warmup)]
    if tree:
        args += ["--tree", tree]
    if ref_threads:
        args += ["--ref-threads", str(ref_threads)]
    if clock:
        args.append("--clock")
    out = child(args, env={"FD_ED25519_LIB": lib} if lib else None, limit=limit)
    line = [x for x in out.splitlines() if x.startswith("SHA_BENCH ")][-1]
    return json.loads(line[len("SHA_BENCH "):])


def run(a):
    def emit(kind, **kw):
        rec = {"tool": "sha_bench", "kind": kind, **kw}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    KB = 1024
    what = set(a.only.split(",")) if a.only else {"long_abs", "short_ab", "pingpong_ab", "bench_ab"}
    if "long_abs" in what:
        for n, sz in ((64, 256 * KB), (1024, 256 * KB), (4096, 256 * KB), (1, 64 * KB * KB)):
            r = run_leg(n, sz, a.reps, 1, ref_threads=16, clock=True)
            emit("long_abs", n=n, sz=sz, gb_per_s=stats(r["gb_per_s"]), seconds=r["seconds"], ref_threads=16,
                 ref_gb_per_s=stats(r["ref_gb_per_s"]), pool_effective_clock_ghz=r.get("pool_effective_clock_ghz"), kernels_id=r["kernels_id"])
    if "short_ab" in what and a.parent:
        ab = {"tree": [], "parent": []}
        clk = None
        for p in range(a.pairs):
            for who in (("tree", "parent") if p % 2 == 0 else ("parent", "tree")):
                r = run_leg(262144, KB, 1, 1, tree=a.parent if who == "parent" else None, clock=(p == 0 and who == "tree"))
                ab[who] += r["seconds"]
                clk = r.get("pool_effective_clock_ghz", clk) if who == "tree" and p == 0 else clk
        lo, hi = max(min(ab["tree"]), min(ab["parent"])), min(max(ab["tree"]), max(ab["parent"]))
        emit("short_ab", n=262144, sz=KB, pairs=a.pairs, tree_seconds=ab["tree"], parent_seconds=ab["parent"], ranges_overlap=lo <= hi,
             pool_effective_clock_ghz=clk)
    if "pingpong_ab" in what and a.pp0_lib:
        for n, sz in ((4096, 256 * KB), (1, 64 * KB * KB)):
            ab = {"pp1": [], "pp0": []}
            clk = None
            for p in range(a.pairs):
                for who in (("pp1", "pp0") if p % 2 == 0 else ("pp0", "pp1")):
                    r = run_leg(n, sz, 1, 1, lib=a.pp0_lib if who == "pp0" else None, clock=(p == 0 and who == "pp1"))
                    ab[who] += r["seconds"]
                    clk = r.get("pool_effective_clock_ghz", clk) if who == "pp1" and p == 0 else clk
            emit("pingpong_ab", n=n, sz=sz, pairs=a.pairs, pingpong_seconds=ab["pp1"], single_buffer_seconds=ab["pp0"],
                 every_pingpong_run_beats_every_single=max(ab["pp1"]) < min(ab["pp0"]), pool_effective_clock_ghz=clk)
    if "bench_ab" in what and a.parent:
        ab = {"tree": [], "parent": []}
        clk = []
        for p in range(a.bench_pairs):
            for who in (("tree", "parent") if p % 2 == 0 else ("parent", "tree")):
                d = a.parent if who == "parent" else ROOT
                out = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=d, limit=600)
                j = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
                ab[who].append(j.get("value"))
                clk.append(find_key(j, "effective_clock_ghz"))
        emit("bench_ab", cmd="bench.py --gpus 1 --steps 20 --warmup 5", pairs=a.bench_pairs, tree_values=ab["tree"], parent_values=ab["parent"],
             clocks=clk)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    lg = sub.add_parser("leg")
    lg.add_argument("--tree")
    lg.add_argument("--n", type=int, required=True)
    lg.add_argument("--sz", type=int, required=True)
    lg.add_argument("--reps", type=int, default=3)
    lg.add_argument("--warmup", type=int, default=1)
    lg.add_argument("--ref-threads", type=int, default=0)
    lg.add_argument("--clock", action="store_true")
    rn = sub.add_parser("run")
    rn.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_sha_long.jsonl"))
    rn.add_argument("--parent", help="a built checkout of the parent commit")
    rn.add_argument("--pp0-lib", help="a library built with -DFD_SHA_LONG_PINGPONG=0")
    rn.add_argument("--pairs", type=int, default=7)
    rn.add_argument("--bench-pairs", type=int, default=3)
    rn.add_argument("--reps", type=int, default=3)
    rn.add_argument("--only", help="comma list of long_abs,short_ab,pingpong_ab,bench_ab")
    a = ap.parse_args()
    (leg if a.cmd == "leg" else run)(a)


if __name__ == "__main__":
    main()
