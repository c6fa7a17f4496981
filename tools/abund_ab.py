#!/usr/bin/env python3
"""abund_ab.py -- what the abundance step costs on the device (k_abund.hip, mtsv_fold_abundance), beside one host thread doing
the same iterations from downloaded records and beside a plain copy of the record bytes.

    timeout -k 10 500 python tools/abund_ab.py [--reads 2000000] [--species 4096] [--rounds 3] [--iters 20] [--skew 1.2]

The workload is synthetic: --reads reads of 1 to 8 records each (2.9 on average) over --species TaxIDs drawn from a Zipf-like
law of exponent --skew, so that a few taxa are in most reads -- the case the LDS counters are for -- with edits 0 to 3.  The
records go into a fold through mtsv_fold_add_records.

The device arm is mtsv_fold_abundance with an output fold and the rows, tol 0 so that all --iters iterations run, --rounds
times after one warm-up, split by its own MTSV_ABUND_TIMING line into prepare, the step kernels, the delta kernels and the
final kernel; once with the adds through LDS (the default when the union fits) and once with MTSV_ABUND_DENSE_MAX=0, every add
a global atomic.  Arm (a): numpy on one thread over the downloaded records, exact in 64-bit integers -- the 96-bit product by
halves, the sums by 16-bit limbs -- its masses and assignments compared with the device's.  Arm (b): hipMemcpyDtoD of the
record bytes."""
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

TAX0 = 1_000_000
STEPS = ("prepare", "step", "delta", "final", "call")


def make_records(n_reads, n_species, skew, seed=1):
    rng = np.random.default_rng(seed)
    count = rng.choice(np.arange(1, 9), size=n_reads, p=[0.35, 0.2, 0.15, 0.1, 0.08, 0.06, 0.04, 0.02])
    read = np.repeat(np.arange(n_reads, dtype=np.uint64), count)
    p = 1.0 / np.arange(1, n_species + 1) ** skew
    species = rng.choice(n_species, size=len(read), p=p / p.sum())
    a = np.zeros(len(read), dtype=M.ASSIGN_DTYPE)
    a["read"], a["tax_id"], a["edit"] = read, TAX0 + species, rng.integers(0, 4, size=len(read))
    a = a[np.lexsort((a["tax_id"], a["read"]))]
    keep = np.ones(len(a), dtype=bool)
    keep[1:] = (a["read"][1:] != a["read"][:-1]) | (a["tax_id"][1:] != a["tax_id"][:-1])  # (keys must be distinct)
    return a[keep]


def host_em(rec, w, iters):
    """numpy on one thread, slack all: (taxa, masses after `iters` iterations, assigned records); exact, as the definition"""
    w = np.asarray(w, dtype=np.uint64)
    head = np.ones(len(rec), dtype=bool)
    head[1:] = rec["read"][1:] != rec["read"][:-1]
    start = np.flatnonzero(head)
    seg = np.cumsum(head) - 1
    edit = rec["edit"].astype(np.int64)
    d = edit - np.minimum.reduceat(edit, start)[seg]
    weight = np.where(d == 0, np.uint64(1 << 32), w[np.minimum(np.maximum(d, 1), len(w)) - 1])
    taxa, slot = np.unique(rec["tax_id"], return_inverse=True)
    mass = np.full(len(taxa), 1 << 32, dtype=np.uint64)

    def x_of(mass):
        a = mass[slot]
        return ((a >> np.uint64(32)) * weight + (((a & np.uint64(0xffffffff)) * weight) >> np.uint64(32))) >> np.uint64(16)

    for _ in range(iters):
        x = x_of(mass)
        s = np.add.reduceat(x, start)
        if not s.all():
            sys.exit("abund_ab: a read whose x sum to zero (the host arm has no fallback)")
        q = ((x.astype(np.float64) / s[seg].astype(np.float64)) * 4294967296.0).astype(np.uint64)
        low = np.bincount(slot, weights=(q & np.uint64(0xffff)).astype(np.float64), minlength=len(taxa))   # (sums below 2^53: exact)
        high = np.bincount(slot, weights=(q >> np.uint64(16)).astype(np.float64), minlength=len(taxa))
        mass = low.astype(np.uint64) + (high.astype(np.uint64) << np.uint64(16))
    x = x_of(mass)
    top = np.maximum.reduceat(x, start)
    first = np.flatnonzero(x == top[seg])                       # (records ascend by TaxID: the first of a read's maxima)
    first = first[np.concatenate(([True], seg[first][1:] != seg[first][:-1]))]
    return taxa, mass, rec[first]


def device_arm(rec, n_reads, w, iters, rounds, dense_max):
    if dense_max is None:
        os.environ.pop("MTSV_ABUND_DENSE_MAX", None)
    else:
        os.environ["MTSV_ABUND_DENSE_MAX"] = str(dense_max)
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=n_reads)  # (the knob is read here)
    fold.add_records(rec)
    out = M.Fold(0, M.GRAIN_TAXID)
    times = {s: [] for s in STEPS}
    facts = None
    for r in range(rounds + 1):  # (call 0 allocates and warms up)
        with Stderr() as err:
            rows, info, ms = fold.abundance(w, slack=M.SLACK_ALL, max_iters=iters, tol=0, out=out)
        m = re.search(r"\[abundance timing\] records (\d+) reads (\d+) entries (\d+) taxa (\d+) listed (\d+) dense (\d) blocks (\d+) iterations (\d+); "
                      + ", ".join(f"{s} ([\\d.]+) ms" for s in STEPS), err.text)
        if not m:
            sys.exit(f"abund_ab: no timing line in: {err.text!r}")
        facts = m.groups()[:8]
        if r:
            for s, x in zip(STEPS, m.groups()[8:]):
                times[s].append(float(x))
    got = out.download()
    fold.close()
    out.close()
    return times, facts, rows, info, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--species", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skew", type=float, default=1.2)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("abund_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_ABUND_TIMING"] = "1"
    w = M.abundance_weights(0.25, 64)
    rec = make_records(args.reads, args.species, args.skew)
    n_bytes = len(rec) * M.ASSIGN_DTYPE.itemsize
    share = np.sort(np.bincount((rec["tax_id"] - TAX0).astype(np.int64)))[::-1]
    print(f"{len(rec)} records ({n_bytes} bytes) of {len(np.unique(rec['read']))} reads over {len(np.unique(rec['tax_id']))} TaxIDs; the 8 most frequent "
          f"hold {share[:8].sum() / len(rec) * 100:.1f}% of the records; {args.iters} iterations, tol 0", flush=True)
    results = {}
    for name, dense_max in (("LDS adds", None), ("global adds", 0)):
        times, facts, rows, info, got = device_arm(rec, args.reads, w, args.iters, args.rounds, dense_max)
        results[name] = (times, rows, info, got)
        n_iter = max(int(facts[7]), 1)
        print(f"device, {name} (dense {facts[5]}, {facts[6]} workgroups, {facts[4]} reads listed, {facts[2]} entries):", flush=True)
        for s in STEPS[:4]:
            per = f"; per iteration {np.mean(times[s]) / n_iter:.4f} ms" if s in ("step", "delta") else ""
            print(f"  {s:8s} {spread(times[s])} ms{per}", flush=True)
        kernels = [sum(times[s][k] for s in STEPS[:4]) for k in range(args.rounds)]
        print(f"  kernels {spread(kernels)} ms, whole call {spread(times['call'])} ms", flush=True)
    a, b = results["LDS adds"], results["global adds"]
    same_tiers = a[1].tolist() == b[1].tolist() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes()
    print(f"step kernel, LDS adds over global adds: {np.mean(a[0]['step']) / np.mean(b[0]['step']):.2f} of the time; results identical: {same_tiers}", flush=True)
    copy_ms = dtod_ms(n_bytes)
    kernels = np.mean([sum(a[0][s][k] for s in STEPS[:4]) for k in range(args.rounds)])
    print(f"(b) hipMemcpyDtoD of the {n_bytes} record bytes: {copy_ms:.3f} ms: one step takes {np.mean(a[0]['step']) / max(a[2]['iterations'], 1) / copy_ms:.2f} times "
          f"the copy, the call's kernels {kernels / copy_ms:.2f} times", flush=True)

    # ---- arm (a): one host thread, from the downloaded records ----
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=args.reads)
    fold.add_records(rec)
    t0 = time.perf_counter()
    down = fold.download()
    t1 = time.perf_counter()
    taxa, mass, assigned = host_em(down, w, args.iters)
    t2 = time.perf_counter()
    fold.close()
    rows, info, got = a[1], a[2], a[3]
    same = rows["tax_id"].tolist() == taxa.tolist() and rows["mass"].tolist() == mass.tolist() and got.tobytes() == assigned.tobytes()
    host_ms = (t2 - t0) * 1e3
    print(f"(a) one host thread: download {(t1 - t0) * 1e3:.3f} ms, numpy {(t2 - t1) * 1e3:.3f} ms ({(t2 - t1) * 1e3 / max(args.iters, 1):.3f} per iteration): "
          f"{host_ms / np.mean(a[0]['call']):.1f} times the device call, {host_ms / kernels:.1f} times its kernels; masses and assignments identical: {same}", flush=True)
    if not (same and same_tiers):
        sys.exit("abund_ab: the arms disagree")


if __name__ == "__main__":
    main()
