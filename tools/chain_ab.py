#!/usr/bin/env python3
"""chain_ab.py -- what handing a run's unmatched reads to a second workspace on the device (k_compact.hip,
mtsv_batch_take_reads) costs, beside what it replaces inside one process.

    timeout -k 10 900 python tools/chain_ab.py [--workload config2] [--filter-workload config1] [--steps 10] [--warmup 3] [--rounds 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/chain_ab.py --trace-run

Two indexes resident on one device: the database D (bench.py's index of --workload) and a filter F (bench.py's index of
--filter-workload).  A step's reads are those of D's workload, every other one sampled from F and the others from D
(mtsv_synth_reads: a tenth of each random), so that the filter drops about 45 % of them.  Two ways through a step, in turn,
--rounds times --steps steps each, in one process on one box:

  (a) chain     F: mtsv_batch_run_host (flags only) -> D: mtsv_batch_take_reads, mtsv_batch_run, mtsv_batch_download
  (b) host      F: mtsv_batch_run_host (flags only), mtsv_batch_match_flags to the host, the survivors packed on the host
                (one numpy take over fixed-length rows, into page-locked memory: the cheapest a host can do it),
                D: mtsv_batch_upload, mtsv_batch_run, mtsv_batch_download

Both end with the same hits (checked once, read numbers translated).  Printed: every round's mean and every step; per way the
time per step and of its hand-over alone (take_reads against flags + packing + upload); the device time of the compaction
kernels (device_ms of mtsv_batch_take_reads) beside a hipMemcpyDtoD of as many bytes as survive, timed with HIP events in the
same process; the bytes each hand-over moves over PCIe.

--trace-run: one warm-up and three chain steps, for a kernel trace."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from report_ab import load_index  # noqa: E402  (bench.py's index file, built and written when it is not there)


def dtod_ms(n_bytes, repeats=5):
    """device time of hipMemcpyDtoD of n_bytes, the fastest of `repeats` after one warm-up (HIP events)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = ctypes.c_void_p

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"chain_ab: {what} failed with HIP error {rc}")

    a, b, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(ctypes.byref(a), ctypes.c_size_t(max(n_bytes, 1))), "hipMalloc")
    ok(hip.hipMalloc(ctypes.byref(b), ctypes.c_size_t(max(n_bytes, 1))), "hipMalloc")
    ok(hip.hipMemset(a, 1, ctypes.c_size_t(n_bytes)), "hipMemset")
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
    best = None
    for k in range(repeats + 1):
        ok(hip.hipEventRecord(e0, None), "hipEventRecord")
        ok(hip.hipMemcpyDtoDAsync(b, a, ctypes.c_size_t(n_bytes), None), "hipMemcpyDtoDAsync")
        ok(hip.hipEventRecord(e1, None), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
        if k and (best is None or ms.value < best):
            best = ms.value
    for p in (a, b):
        hip.hipFree(p)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--filter-workload", default="config1")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("chain_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    ix_d, n_reads, read_len, desc_d = load_index(args.workload)
    ix_f, _, _, desc_f = load_index(args.filter_workload)
    if args.reads:
        n_reads = args.reads
    n_reads -= n_reads % 2
    half = n_reads // 2
    from_f, _ = M.synth_reads(ix_f, seed=1001, n_reads=half, read_len=read_len)
    from_d, _ = M.synth_reads(ix_d, seed=1000, n_reads=half, read_len=read_len)
    pinned = M.HostBuffer(n_reads * read_len)
    rows = pinned.array.reshape(n_reads, read_len)
    rows[0::2] = from_f.reshape(half, read_len)
    rows[1::2] = from_d.reshape(half, read_len)
    del from_f, from_d
    bases = pinned.array
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    print(f"database {args.workload}: {desc_d}; filter {args.filter_workload}: {desc_f}; {n_reads} reads of {read_len} bases per step", flush=True)
    params = M.default_params()
    slice_reads = M.bin_batch_slice_reads(n_reads)
    src = M.Batch(ix_f, 0, min(n_reads, slice_reads), min(len(bases), slice_reads * (read_len + 8)))
    src.set_match_flags(M.MATCH_ONLY)
    dst = M.Batch(ix_d, 0, n_reads, len(bases))
    packed = M.HostBuffer(n_reads * read_len)
    packed_rows = packed.array.reshape(n_reads, read_len)

    def chain_step():
        t0 = time.perf_counter()
        src.run_host(bases, off, params)
        t1 = time.perf_counter()
        n_kept, bases_kept, ms = dst.take_reads(src, M.KEEP_UNMATCHED)
        t2 = time.perf_counter()
        dst.run(params)
        hits = dst.download()
        t3 = time.perf_counter()
        return hits, dict(step=(t3 - t0) * 1e3, filter=(t1 - t0) * 1e3, hand_over=(t2 - t1) * 1e3, run=(t3 - t2) * 1e3, n_kept=n_kept,
                          bases_kept=bases_kept, device_ms=ms, d2h=24 + 4 * (n_kept + 1), h2d=0)

    def host_step():
        t0 = time.perf_counter()
        src.run_host(bases, off, params)
        t1 = time.perf_counter()
        flags, _ = src.match_flags()
        keep = np.flatnonzero(~flags)
        np.take(rows, keep, axis=0, out=packed_rows[:len(keep)])
        dst.upload(packed.array[:len(keep) * read_len], off[:len(keep) + 1])
        t2 = time.perf_counter()
        dst.run(params)
        hits = dst.download()
        t3 = time.perf_counter()
        return (hits, keep), dict(step=(t3 - t0) * 1e3, filter=(t1 - t0) * 1e3, hand_over=(t2 - t1) * 1e3, run=(t3 - t2) * 1e3, n_kept=len(keep),
                                  bases_kept=len(keep) * read_len, device_ms=0.0, d2h=8 * ((n_reads + 63) // 64) + 8, h2d=len(keep) * (read_len + 4) + 4)

    if args.trace_run:
        for _ in range(4):
            hits, f = chain_step()
        print(f"trace run: one warm-up and three chain steps, {f['n_kept']} of {n_reads} reads kept, {len(hits)} hits per step", flush=True)
        return

    # the two ways end with the same hits
    hits_a, fa = chain_step()
    (hits_b, keep), fb = host_step()
    hits_b = hits_b.copy()
    hits_b["read"] = keep[hits_b["read"].astype(np.int64)]
    same = len(hits_a) == len(hits_b) and all(np.array_equal(hits_a[f], hits_b[f]) for f in M.HIT_DTYPE.names)
    print(f"{fa['n_kept']} of {n_reads} reads survive the filter ({fa['bases_kept']} bases); {len(hits_a)} hits in the database; "
          f"hits of the two ways identical: {same}", flush=True)
    if not same or fa["n_kept"] != fb["n_kept"]:
        sys.exit("chain_ab: the chain and the host hand-over disagree")

    ways = (("chain", chain_step), ("host", host_step))
    means = {name: [] for name, _ in ways}
    parts = {name: [] for name, _ in ways}
    for r in range(1, args.rounds + 1):
        for name, step in ways:
            for _ in range(args.warmup if r == 1 else 1):
                step()
            each = [step()[1] for _ in range(args.steps)]
            parts[name] += each
            m = sum(f["step"] for f in each) / len(each)
            means[name].append(m)
            print(f"round {r} {name:5s} ms_per_step {m:8.3f}  steps: " + " ".join(f"{f['step']:.2f}" for f in each), flush=True)
    copy_ms = dtod_ms(fa["bases_kept"])
    for name, _ in ways:
        p = parts[name]
        mean = lambda k: float(np.mean([f[k] for f in p]))  # noqa: E731
        print(f"{name:5s}: {np.mean(means[name]):8.3f} ms per step (rounds {min(means[name]):.3f}..{max(means[name]):.3f}): filter run {mean('filter'):.3f}, "
              f"hand-over {mean('hand_over'):.3f}, database run + download {mean('run'):.3f}; per hand-over {p[-1]['d2h']} bytes to the host, "
              f"{p[-1]['h2d']} to the device", flush=True)
    dev = [f["device_ms"] for f in parts["chain"]]
    nb = fa["bases_kept"]
    src_bytes = n_reads * read_len
    print(f"compaction kernels: {np.mean(dev):.3f} ms of device time per hand-over (min {min(dev):.3f}, max {max(dev):.3f}) for {nb} surviving bytes "
          f"out of {src_bytes}; hipMemcpyDtoD of {nb} bytes: {copy_ms:.3f} ms ({nb / copy_ms / 1e6:.0f} GB/s); the kernels take "
          f"{np.mean(dev) / copy_ms:.2f} times the plain copy and move {(2 * nb + 8 * (n_reads + 1)) / np.mean(dev) / 1e6:.0f} GB/s "
          f"(survivors read and written once, the offsets read twice)", flush=True)
    for b in (src, dst):
        b.close()
    pinned.close()
    packed.close()


if __name__ == "__main__":
    main()
