#!/usr/bin/env python3
"""report_ab.py -- what the taxa report (k_report.hip) costs a step, measured through the library as bench.py does.

    python tools/report_ab.py [--workload config2] [--steps 20] [--warmup 5] [--rounds 3]
    MTSV_LANES=1 MTSV_TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/report_ab.py --trace-run uniform|skewed

The same index file, reads and workspaces as bench.py's timed region (host path: mtsv_batch_run_host + mtsv_batch_download on
reads in page-locked memory) and its `device_resident` leg (mtsv_batch_run on reads in HBM).  Report off and report on
alternate, --rounds times --steps steps each, in one process; every round's mean and every step are printed, then the
difference of the means beside the off-rounds' spread (a difference below twice that spread cannot be told apart).  The same
once more on a skewed input: every read of the step taken from the reads of the uniform batch that hit the batch's most
frequent TaxID (repeated to the batch's size), so that nearly every add of a pass lands on one taxon's counters.

--trace-run: one warm-up and three passes of one input through a resident workspace with the report on, for a kernel trace
(k_report beside k_gather); with MTSV_TRACE the library prints the kernel's launches and its atomic adds on the global counters."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload table, seeds, index file name)
import mtsv_tools_amd as M  # noqa: E402
from mtsv_tools_amd import _lib as L  # noqa: E402


def load_index(workload):
    n_taxa, gis, seq_len, n_reads, read_len, desc = bench.WORKLOADS[workload]
    path = f"/tmp/mtsv_bench_{workload}.idx"
    expect_n = n_taxa * gis * seq_len + 1
    cached = False
    try:
        cached = os.path.exists(path) and int.from_bytes(open(path, "rb").read(8), "little") == expect_n
    except OSError:
        pass
    if not cached:
        M.set_build_device(0)
        ix = M.MGIndex.synth(bench.SEED_DB, n_taxa, gis, seq_len, threads=min(32, os.cpu_count() or 8))
        M.set_build_device(-1)
        ix.write(path + ".tmp")
        os.replace(path + ".tmp", path)
        print("index file written", flush=True)
    else:
        ix = M.MGIndex.load(path)
    ix.to_device(0, 0)
    return ix, n_reads, read_len, desc


def skewed_from(ix, bases, off, n_reads, read_len):
    """the reads of the uniform batch that hit its most frequent TaxID, repeated to n_reads reads"""
    hits = ix.bin_batch(bases, off, M.default_params(), device=0)
    tax, cnt = np.unique(hits["tax_id"], return_counts=True)
    t = int(tax[np.argmax(cnt)])
    idx = np.unique(hits["read"][hits["tax_id"] == t]).astype(np.int64)
    out = bases.reshape(n_reads, read_len)[np.resize(idx, n_reads)].reshape(-1).copy()
    return out, t, len(idx)


def rounds(label, step, set_report, args):
    means = {False: [], True: []}
    for r in range(1, args.rounds + 1):
        for on in (False, True):
            set_report(on)
            for _ in range(args.warmup if r == 1 else 2):
                step()
            each = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                step()
                each.append((time.perf_counter() - t0) * 1e3)
            m = sum(each) / len(each)
            means[on].append(m)
            print(f"{label} round {r} report {'on ' if on else 'off'} ms_per_step {m:7.3f}  steps: " + " ".join(f"{x:.2f}" for x in each), flush=True)
    off_m, on_m = np.mean(means[False]), np.mean(means[True])
    spread = max(means[False]) - min(means[False])
    print(f"{label}: off {off_m:.3f} ms (rounds {min(means[False]):.3f}..{max(means[False]):.3f}, spread {spread:.3f}), on {on_m:.3f} ms "
          f"(rounds {min(means[True]):.3f}..{max(means[True]):.3f}); on - off = {on_m - off_m:+.3f} ms, twice the off spread = {2 * spread:.3f} ms", flush=True)


def ab(ix, bases, off, n_reads, read_len, label, args):
    params = M.default_params()
    slice_reads = M.bin_batch_slice_reads(n_reads)
    hb = M.Batch(ix, 0, min(n_reads, slice_reads), min(len(bases), slice_reads * (read_len + 8)))
    pinned = M.HostBuffer(len(bases))
    pinned.array[:] = bases
    bases_p, off_p = pinned.array.ctypes.data, off.ctypes.data

    def host_step():
        L._check(M.lib().mtsv_batch_run_host(hb.h, bases_p, off_p, n_reads, ctypes.byref(params)))
        out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
        L._check(M.lib().mtsv_batch_download(hb.h, ctypes.byref(out_p), ctypes.byref(out_n)))
        M.lib().mtsv_hits_free(out_p)

    rounds(f"{label} host path", host_step, hb.set_taxa_report, args)
    hb.set_taxa_report(True)
    rows, total, ms = hb.taxa_report(reset=True)
    host_step()
    rows, total, ms = hb.taxa_report()
    top = rows[np.argmax(rows["only_hit"] + rows["only_best"] + rows["tied_best"] + rows["not_best"])]
    print(f"{label} host path, one step with the report on: k_report {ms:.3f} ms of device time, {len(rows)} rows, total_reads {total}, "
          f"largest row tax_id {top['tax_id']}: {top['only_hit']} {top['only_best']} {top['tied_best']} {top['not_best']}", flush=True)
    hb.close()
    pinned.close()
    rb = M.Batch(ix, 0, n_reads, len(bases))
    rb.upload(bases, off)
    rounds(f"{label} resident  ", lambda: rb.run(params), rb.set_taxa_report, args)
    rb.close()


def trace_run(ix, bases, off, n_reads, label):
    b = M.Batch(ix, 0, n_reads, len(bases))
    b.set_taxa_report(True)
    b.upload(bases, off)
    b.run()
    b.taxa_report(reset=True)
    for _ in range(3):
        b.run()
    rows, total, ms = b.taxa_report()
    st = b.stats()
    print(f"{label}: 3 passes, n_lanes {st['n_lanes']}, n_passes of the last run {st['n_passes']}, k_report {ms / 3:.3f} ms per run by HIP events, "
          f"gather stage {st['stage_ms']['gather']:.3f} ms, {len(rows)} rows, total_reads {total}", flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--trace-run", choices=["uniform", "skewed"], default=None)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("report_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    ix, n_reads, read_len, desc = load_index(args.workload)
    if args.reads:
        n_reads = args.reads
    bases, off = M.synth_reads(ix, seed=1000, n_reads=n_reads, read_len=read_len)
    print(f"{args.workload}: {desc}; {n_reads} reads per step", flush=True)
    if args.trace_run != "uniform":
        sk, t, n_src = skewed_from(ix, bases, off, n_reads, read_len)
        print(f"skewed input: the {n_src} reads of the uniform batch with a hit on TaxID {t}, repeated to {n_reads} reads", flush=True)
    if args.trace_run:
        return trace_run(ix, bases if args.trace_run == "uniform" else sk, off, n_reads, args.trace_run)
    ab(ix, bases, off, n_reads, read_len, "uniform", args)
    ab(ix, sk, off, n_reads, read_len, "skewed ", args)


if __name__ == "__main__":
    main()
