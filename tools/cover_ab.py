#!/usr/bin/env python3
"""cover_ab.py -- what coverage per reference costs on the device (k_cover.hip, mtsv_coverage), beside one host thread doing
the same from downloaded records, beside a plain copy of the record bytes, and beside mtsv_fold_taxa_report on the same fold.

    timeout -k 10 500 python tools/cover_ab.py [--reads 1000000] [--slack 0] [--rounds 5]

The workload is binned, not made up: a synthetic index (64 taxa, 2 GIs each, 50,000 bases a sequence), --reads reads of 100
bases from mtsv_synth_reads (one in ten random, the rest with the noise that call adds), run at MTSV_GRAIN_LONG and folded with
mtsv_fold_add_run.

The device arm is mtsv_coverage_reset + _add_fold + _rows, --rounds times after one warm-up, split by their own
MTSV_COVER_TIMING lines into bounds, min, map (with the scan of the heads), mark, wave, reads, and the popcount of rows.  Arm (a):
numpy on one thread over the downloaded records -- the reads' minima by reduceat, the references by searchsorted, the covered
bases by a difference array over all positions -- its rows compared with the device's.  Arm (b): hipMemcpyDtoD of the record
bytes.  Arm (c): mtsv_fold_taxa_report on the same fold, device time."""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402
from lca_ab import Stderr, spread  # noqa: E402

READ_LEN = 100
STEPS = ("bounds", "min", "map", "mark", "wave", "reads", "call")


def host_rows(rec, read_len, table, slack):
    """numpy on one thread: the rows mtsv_coverage_rows gives, as a REF_COVERAGE_DTYPE array with the table's references"""
    out = table.copy()
    for name in ("reads", "alignments", "aligned_bases", "covered_bases"):
        out[name] = 0
    if not len(rec):
        return out
    read, edit = rec["read"].astype(np.int64), rec["edit"].astype(np.int64)
    first = np.flatnonzero(np.r_[True, read[1:] != read[:-1]])
    best = np.repeat(np.minimum.reduceat(edit, first), np.diff(np.r_[first, len(rec)]))
    counted = edit <= np.minimum(best + slack, 0xffffffff)
    keys = (table["tax_id"].astype(np.uint64) << np.uint64(32)) | table["gi"].astype(np.uint64)
    ref = np.searchsorted(keys, (rec["tax_id"].astype(np.uint64) << np.uint64(32)) | rec["gi"].astype(np.uint64))
    length = table["length"].astype(np.int64)
    start = rec["offset"].astype(np.int64)
    end = np.minimum(start + read_len[read].astype(np.int64), length[ref])
    run_head = np.r_[True, (read[1:] != read[:-1]) | (ref[1:] != ref[:-1])]
    run = np.cumsum(run_head) - 1
    hit_runs = np.unique(run[counted])
    run_ref = ref[run_head]
    n = len(table)
    out["reads"] = np.bincount(run_ref[hit_runs], minlength=n)
    out["alignments"] = np.bincount(ref[counted], minlength=n)
    out["aligned_bases"] = np.bincount(ref[counted], weights=(end - start)[counted], minlength=n).astype(np.uint64)
    base = np.r_[0, np.cumsum(length)]
    diff = np.zeros(base[-1] + 1, dtype=np.int32)
    np.add.at(diff, (base[ref] + start)[counted], 1)
    np.add.at(diff, (base[ref] + end)[counted], -1)
    covered = np.r_[0, np.cumsum(np.cumsum(diff[:-1]) > 0)]
    out["covered_bases"] = covered[base[1:]] - covered[base[:-1]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--slack", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("cover_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_COVER_TIMING"] = "1"
    ix = M.MGIndex.synth(seed=5, n_taxa=64, gis_per_taxon=2, seq_len=50000)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=3, n_reads=args.reads, read_len=READ_LEN)
    read_len = np.diff(np.asarray(off, dtype=np.uint64)).astype(np.uint32)
    t0 = time.perf_counter()
    ws = M.Batch(ix, 0, args.reads, len(bases), lanes=1)
    ws.set_assignment_grain(M.GRAIN_LONG)
    ws.set_assignments(M.ASSIGN_ONLY)
    ws.upload(bases, off)
    ws.run()
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=args.reads)
    fold.add_run(ws)
    ws.close()
    n_rec = fold.count()
    n_bytes = n_rec * M.ASSIGN_GI_DTYPE.itemsize
    print(f"{args.reads} reads binned and folded in {time.perf_counter() - t0:.2f} s: {n_rec} records ({n_bytes} bytes) at MTSV_GRAIN_LONG; slack {args.slack}",
          flush=True)

    cov = M.Coverage(0)
    cov.add_index(ix)
    times, pop, rows_call = {s: [] for s in STEPS}, [], []
    rows = None
    for r in range(args.rounds + 1):  # (call 0 lays the table out, allocates and warms up)
        cov.reset()
        with Stderr() as err:
            cov.add_fold(fold, read_len, args.slack)
            rows, _ = cov.rows()
        m = re.search(r"\[cover timing\] add_fold records \d+ reads \d+ runs (\d+) counted (\d+) listed (\d+); " + ", ".join(f"{s} ([\\d.]+) ms" for s in STEPS), err.text)
        p = re.search(r"\[cover timing\] rows references (\d+) words (\d+) tile \d+; popcount ([\d.]+) ms, call ([\d.]+) ms", err.text)
        if not m or not p:
            sys.exit(f"cover_ab: no timing lines in: {err.text!r}")
        if r:
            for s, x in zip(STEPS, m.groups()[3:]):
                times[s].append(float(x))
            pop.append(float(p.group(3)))
            rows_call.append(float(p.group(4)))
    print(f"{p.group(1)} references in a bitmap of {p.group(2)} words; {m.group(1)} (read, reference) runs, {m.group(2)} records counted, {m.group(3)} on the "
          f"wavefront tier's work list; {int((rows['alignments'] > 0).sum())} references hit, {int(rows['covered_bases'].sum())} bases covered", flush=True)
    kernels = [sum(times[s][k] for s in STEPS[:6]) for k in range(args.rounds)]
    for s in STEPS[:6]:
        print(f"  {s:8s} {spread(times[s])} ms", flush=True)
    print(f"device: add_fold kernels {spread(kernels)} ms, whole call {spread(times['call'])} ms; rows popcount {spread(pop)} ms, whole call {spread(rows_call)} ms",
          flush=True)
    copy_ms = dtod_ms(n_bytes)
    print(f"(b) hipMemcpyDtoD of the {n_bytes} record bytes: {copy_ms:.3f} ms: the add_fold kernels take {np.mean(kernels) / copy_ms:.2f} times the copy", flush=True)

    # ---- arm (c): mtsv_fold_taxa_report on the same fold ----
    report_ms = []
    for r in range(args.rounds + 1):
        _, _, ms = fold.taxa_report()
        if r:
            report_ms.append(ms)
    slowest = max(STEPS[:6], key=lambda s: np.mean(times[s]))
    print(f"(c) mtsv_fold_taxa_report on the same fold: kernels {spread(report_ms)} ms: add_fold takes {np.mean(kernels) / np.mean(report_ms):.2f} times that; its "
          f"longest step is {slowest} ({np.mean(times[slowest]):.3f} ms)", flush=True)

    # ---- arm (a): one host thread, from the downloaded records ----
    host = []
    for r in range(min(args.rounds, 3)):
        t0 = time.perf_counter()
        down = fold.download_gi()
        t1 = time.perf_counter()
        want = host_rows(down, read_len, rows, args.slack)
        host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    same = rows.tobytes() == want.tobytes()
    both = [a + b for a, b in host]
    device = np.mean(times["call"]) + np.mean(rows_call)
    print(f"(a) one host thread: download {spread([a for a, _ in host])} ms, numpy {spread([b for _, b in host])} ms: {np.mean(both) / device:.1f} times the two "
          f"device calls, {np.mean(both) / (np.mean(kernels) + np.mean(pop)):.1f} times their kernels; rows identical: {same}", flush=True)
    fold.close()
    cov.close()
    if not same:
        sys.exit("cover_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
