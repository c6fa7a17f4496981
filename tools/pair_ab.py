#!/usr/bin/env python3
"""pair_ab.py -- what joining the mates' assignments costs on the device (k_pair.hip, mtsv_fold_pair), beside one host thread
doing the same join from downloaded records, beside a plain copy of the record bytes, and beside mtsv_fold_lca on the same fold.

    timeout -k 10 500 python tools/pair_ab.py [--pairs 500000] [--mode proper|both|either] [--max-insert 513] [--rounds 5]

The workload is binned, not made up: a synthetic index (64 taxa, 2 GIs each, 50,000 bases a sequence), --pairs fragments of 400
bases from mtsv_synth_reads (one in ten random, the rest with the noise that call adds), mate 1 the first 100 bases and mate 2
the reverse complement of the last 100, interleaved, run at MTSV_GRAIN_LONG and folded with mtsv_fold_add_run.

The device arm is mtsv_fold_pair, --rounds times after one warm-up, split by its own MTSV_PAIR_TIMING line into bounds, the
join's lane tier, its wavefront tier, reduce (heads, scan, segmented minimum, flags, scans), write (with the merge of the two
lists in `either`) and stats.  Arm (a): numpy on one thread over the downloaded records -- the windows by searchsorted, their
minima, the minimum per (pair, TaxID) -- its records compared with the device's.  Arm (b): hipMemcpyDtoD of the record bytes.
Arm (c): mtsv_fold_lca (slack 0, a flat taxonomy) on the same fold, device time."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402
from lca_ab import Stderr, spread  # noqa: E402

FRAGMENT, READ_LEN, UNPAIRED = 400, 100, 7
STEPS = ("bounds", "join", "wave", "reduce", "write", "stats", "call")
MODES = {"both": M.PAIR_BOTH, "either": M.PAIR_EITHER, "proper": M.PAIR_PROPER}
COMP = np.full(256, ord("N"), dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b


def mates_of(ix, n_pairs, seed=3):
    """the interleaved mates of n_pairs fragments as (bases, read_off)"""
    frags, _ = M.synth_reads(ix, seed=seed, n_reads=n_pairs, read_len=FRAGMENT)
    frags = np.asarray(frags, dtype=np.uint8).reshape(n_pairs, FRAGMENT)
    reads = np.empty((n_pairs, 2, READ_LEN), dtype=np.uint8)
    reads[:, 0] = frags[:, :READ_LEN]
    reads[:, 1] = COMP[frags[:, :-READ_LEN - 1:-1]]
    return reads.reshape(-1), np.arange(2 * n_pairs + 1, dtype=np.uint64) * READ_LEN


def segment_min(keys, values):
    """(distinct keys, the smallest value of each) of rows already ordered by key"""
    head = np.ones(len(values), dtype=bool)
    head[1:] = (keys[1:] != keys[:-1]).any(axis=1)
    start = np.flatnonzero(head)
    return keys[start], np.minimum.reduceat(values, start) if len(start) else values[:0]


def host_pair(rec, mode, max_insert):
    """numpy on one thread: the records mtsv_fold_pair gives, as an ASSIGN_DTYPE array"""
    pair, mate = (rec["read"] >> 1).astype(np.int64), (rec["read"] & 1).astype(bool)
    tax, edit = rec["tax_id"].astype(np.int64), rec["edit"].astype(np.int64)
    none = np.int64(1) << 40
    if mode == M.PAIR_PROPER:
        # a number per (pair, tax_id, gi), ascending in key order: the key of a record is (that number, offset)
        grp = np.stack([pair, tax, rec["gi"].astype(np.int64)], axis=1)
        head = np.ones(len(rec), dtype=bool)
        order = np.lexsort((grp[:, 2], grp[:, 1], grp[:, 0]))
        g = grp[order]
        head[1:] = (g[1:] != g[:-1]).any(axis=1)
        gid = np.empty(len(rec), dtype=np.int64)
        gid[order] = np.cumsum(head) - 1
        off = rec["offset"].astype(np.int64)
        i0, i1 = np.flatnonzero(~mate), np.flatnonzero(mate)
        k1 = (gid[i1] << 32) | off[i1]
        by = np.argsort(k1, kind="stable")
        k1, e1 = k1[by], edit[i1][by]
        lo = np.searchsorted(k1, (gid[i0] << 32) | np.maximum(off[i0] - max_insert, 0), "left")
        hi = np.searchsorted(k1, (gid[i0] << 32) | np.minimum(off[i0] + max_insert, 0xffffffff), "right")
        best = np.full(len(i0), none)
        for k in range(int((hi - lo).max()) if len(i0) else 0):
            at = lo + k
            ok = at < hi
            best[ok] = np.minimum(best[ok], e1[at[ok]])
        keep = best < none
        keys, vals = np.stack([pair[i0][keep], tax[i0][keep]], axis=1), (edit[i0] + best)[keep]
        by = np.lexsort((keys[:, 1], keys[:, 0]))
        keys, vals = segment_min(keys[by], vals[by])
    else:
        per = []
        for m in (False, True):
            sel = mate == m
            per.append(segment_min(np.stack([pair[sel], tax[sel]], axis=1), edit[sel]))  # (the list is ordered by (read, tax_id))
        (ka, va), (kb, vb) = per
        code = lambda k: (k[:, 0] << 32) | k[:, 1]  # noqa: E731
        ca, cb = code(ka), code(kb)
        in_b, in_a = np.isin(ca, cb), np.isin(cb, ca)
        both_keys, both_vals = ka[in_b], va[in_b] + vb[in_a]
        if mode == M.PAIR_BOTH:
            keys, vals = both_keys, both_vals
        else:
            keys = np.concatenate([both_keys, ka[~in_b], kb[~in_a]])
            vals = np.concatenate([both_vals, va[~in_b] + UNPAIRED, vb[~in_a] + UNPAIRED])
            by = np.lexsort((keys[:, 1], keys[:, 0]))
            keys, vals = keys[by], vals[by]
    out = np.zeros(len(vals), dtype=M.ASSIGN_DTYPE)
    out["read"], out["tax_id"], out["edit"] = keys[:, 0], keys[:, 1], vals
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--mode", choices=list(MODES), default="proper")
    ap.add_argument("--max-insert", type=int, default=FRAGMENT + 13)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("pair_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_PAIR_TIMING"] = "1"
    os.environ["MTSV_LCA_TIMING"] = "1"
    mode = MODES[args.mode]
    ix = M.MGIndex.synth(seed=5, n_taxa=64, gis_per_taxon=2, seq_len=50000)
    ix.to_device(0)
    bases, off = mates_of(ix, args.pairs)
    n_reads = 2 * args.pairs
    t0 = time.perf_counter()
    ws = M.Batch(ix, 0, n_reads, len(bases), lanes=1)
    ws.set_assignment_grain(M.GRAIN_LONG)
    ws.set_assignments(M.ASSIGN_ONLY)
    ws.upload(bases, off)
    ws.run()
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=n_reads)
    fold.add_run(ws)
    ws.close()
    n_rec = fold.count()
    n_bytes = n_rec * M.ASSIGN_GI_DTYPE.itemsize
    print(f"{args.pairs} pairs binned and folded in {time.perf_counter() - t0:.2f} s: {n_rec} records ({n_bytes} bytes) at MTSV_GRAIN_LONG; mode {args.mode}, "
          f"max_insert {args.max_insert}", flush=True)

    out = M.Fold(0, M.GRAIN_TAXID)
    times = {s: [] for s in STEPS}
    stats = None
    for r in range(args.rounds + 1):  # (call 0 allocates and warms up)
        with Stderr() as err:
            stats, ms = fold.pair(mode, args.max_insert, UNPAIRED, out=out)
        m = re.search(r"\[pair timing\] mode \d+ records \d+ pairs \d+ runs (\d+) listed (\d+) out (\d+); " + ", ".join(f"{s} ([\\d.]+) ms" for s in STEPS), err.text)
        if not m:
            sys.exit(f"pair_ab: no timing line in: {err.text!r}")
        if r:
            for s, x in zip(STEPS, m.groups()[3:]):
                times[s].append(float(x))
    print(f"stats: {stats}; {m.group(1)} (read, TaxID) runs, {m.group(2)} records on the wavefront tier's work list", flush=True)
    kernels = [sum(times[s][k] for s in STEPS[:6]) for k in range(args.rounds)]
    for s in STEPS[:6]:
        print(f"  {s:8s} {spread(times[s])} ms", flush=True)
    print(f"device: kernels {spread(kernels)} ms, whole call {spread(times['call'])} ms", flush=True)
    copy_ms = dtod_ms(n_bytes)
    print(f"(b) hipMemcpyDtoD of the {n_bytes} record bytes: {copy_ms:.3f} ms: the kernels take {np.mean(kernels) / copy_ms:.2f} times the copy", flush=True)

    # ---- arm (c): mtsv_fold_lca on the same fold ----
    taxa = np.unique(fold.download_gi()["tax_id"])
    with tempfile.NamedTemporaryFile("w", suffix=".dmp", delete=False) as fh:
        fh.write("4000000000\t|\t4000000000\t|\troot\t|\n" + "".join(f"{t}\t|\t4000000000\t|\tspecies\t|\n" for t in taxa.tolist()))
    tx = M.Taxonomy(fh.name)
    os.remove(fh.name)
    lca_out, lca_ms = M.Fold(0, M.GRAIN_TAXID), []
    for r in range(args.rounds + 1):
        with Stderr():
            _, _, ms = fold.lca(tx, 0, out=lca_out)
        if r:
            lca_ms.append(ms)
    slowest = max(STEPS[:6], key=lambda s: np.mean(times[s]))
    print(f"(c) mtsv_fold_lca on the same fold: kernels {spread(lca_ms)} ms: the join takes {np.mean(kernels) / np.mean(lca_ms):.2f} times that; its longest step is "
          f"{slowest} ({np.mean(times[slowest]):.3f} ms)", flush=True)

    # ---- arm (a): one host thread, from the downloaded records ----
    host = []
    for r in range(min(args.rounds, 3)):
        t0 = time.perf_counter()
        down = fold.download_gi()
        t1 = time.perf_counter()
        want = host_pair(down, mode, args.max_insert)
        host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    same = out.download().tobytes() == want.tobytes()
    both = [a + b for a, b in host]
    print(f"(a) one host thread: download {spread([a for a, _ in host])} ms, numpy {spread([b for _, b in host])} ms: {np.mean(both) / np.mean(times['call']):.1f} times "
          f"the device call, {np.mean(both) / np.mean(kernels):.1f} times its kernels; records identical: {same}", flush=True)
    for f in (fold, out, lca_out):
        f.close()
    if not same:
        sys.exit("pair_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
