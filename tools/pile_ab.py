#!/usr/bin/env python3
"""pile_ab.py -- what the pileup of a run's hits costs on the device (k_pile.hip, mtsv_pileup), beside one host thread that
builds the same table from downloaded placements, beside a plain copy of the placement and op bytes that such a host thread
needs first, and on a deep pile.

    timeout -k 10 500 python tools/pile_ab.py [--reads 1000000] [--rounds 5] [--host-hits 20000] [--deep-reads 200000]

The workload is binned, not made up: the synthetic index and reads of tools/place_ab.py (64 taxa, 2 GIs each, 50,000 bases a
sequence; --reads reads of 150 bases from mtsv_synth_reads), run resident on one lane.

The device arm is mtsv_pileup_add_run(hits = NULL) into one accumulator, --rounds times after one warm-up call (which learns
the references and allocates the segment), split by its own MTSV_PILE_TIMING line into the placement (map + scan, kernel), the
best-edit pass and the pile kernel; then mtsv_pileup_sites under (1, 1, 0).  Beside it: mtsv_batch_place_hits with its
download, hipMemcpyDtoD of the placement and op bytes, and one host thread walking the ops of --host-hits downloaded placements
into a dict of numpy arrays, scaled to all hits; a second accumulator that is given the same --host-hits hits must hold the
host thread's counters.

The deep pile: --deep-reads reads of 150 bases cut from ONE stretch of 300 bases with 1 % substitutions, binned, and piled
--rounds times: every hit adds to the same few hundred slots."""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mtsv_tools_amd as M  # noqa: E402
import pack_ref  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402
from lca_ab import Stderr, spread  # noqa: E402

READ_LEN = 150
ADD = re.compile(r"\[pile timing\] add_run hits (\d+) piled (\d+) skipped (\d+) op_slots (\d+) new_refs (\d+); place_scan ([\d.]+) ms, place ([\d.]+) ms, "
                 r"best ([\d.]+) ms, pile ([\d.]+) ms, call ([\d.]+) ms")
SITES = re.compile(r"\[pile timing\] sites segments (\d+) slots (\d+) tile (\d+) rows (\d+); sites ([\d.]+) ms, call ([\d.]+) ms")
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def timed_add(p, ws, rounds):
    steps = {s: [] for s in ("place_scan", "place", "best", "pile", "call")}
    m = None
    for r in range(rounds + 1):                                # (call 0 learns the references and allocates)
        with Stderr() as err:
            p.add_run(ws)
        m = ADD.search(err.text)
        if not m:
            sys.exit(f"pile_ab: no timing line in: {err.text!r}")
        if r:
            for s, x in zip(steps, m.groups()[5:]):
                steps[s].append(float(x))
    return steps, m


def host_table(pl, ops, codes, off, lens):
    """one host thread: the placements' ops into {(tax_id, gi): uint32 [L + 1][8]}"""
    table = {}
    for q in pl:
        key = (int(q["tax_id"]), int(q["gi"]))
        t = table.get(key)
        if t is None:
            t = table[key] = np.zeros((lens[key] + 1, 8), dtype=np.uint32)
        r = int(q["read"])
        P = codes[off[r]:off[r + 1]]
        if q["strand"]:
            P = COMP[P[::-1]]
        i, j = 0, int(q["ref_start"])
        for op in ops[int(q["ops_off"]):int(q["ops_off"]) + int(q["n_ops"])].tolist():
            n, c = op >> 4, op & 15
            if c == M.CIGAR_EQ:
                t[j:j + n, 0] += 1
                i, j = i + n, j + n
            elif c == M.CIGAR_X:
                for _ in range(n):
                    t[j, 1 + P[i]] += 1
                    i, j = i + 1, j + 1
            elif c == M.CIGAR_D:
                t[j:j + n, 6] += 1
                j += n
            else:
                t[j, 7] += 1
                i += n
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-hits", type=int, default=20000)
    ap.add_argument("--deep-reads", type=int, default=200_000)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("pile_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_PILE_TIMING"] = "1"
    ix = M.MGIndex.synth(seed=5, n_taxa=64, gis_per_taxon=2, seq_len=50000)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"pile_ab_{os.getpid()}.idx")
    ix.write(path)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=3, n_reads=args.reads, read_len=READ_LEN)
    ws = M.Batch(ix, 0, args.reads, len(bases), lanes=1)
    ws.upload(bases, off)
    ws.run()                                                   # (warms the clocks and the workspace)
    ws.run()
    hits = ws.download()
    print(f"{args.reads} reads of {READ_LEN} bases, {len(hits)} hits; the run {ws.stats()['stage_ms']['total']:.3f} ms", flush=True)

    p = M.Pileup(0)
    steps, m = timed_add(p, ws, args.rounds)
    info = p.info()
    print(f"{m.group(1)} hits, {m.group(2)} piled at slack 0, {m.group(4)} op slots; {info['n_refs']} references, {info['n_slots']} slots, "
          f"{info['device_bytes']} bytes on the device", flush=True)
    for s in steps:
        print(f"  {s:10s} {spread(steps[s])} ms", flush=True)
    with Stderr() as err:
        rows, _ = p.sites(1, 1, 0)
    sm = SITES.search(err.text)
    print(f"  sites      {float(sm.group(5)):.3f} ms for {len(rows)} rows of {sm.group(2)} slots (call {float(sm.group(6)):.3f} ms)", flush=True)

    # ---- what a host thread needs first: the placements and ops on the host ----
    pl, ops, place_ms = ws.place_hits()
    n_bytes = pl.nbytes + ops.nbytes
    print(f"mtsv_batch_place_hits with its download of {n_bytes} bytes: {place_ms:.3f} ms; hipMemcpyDtoD of as many bytes: {dtod_ms(n_bytes):.3f} ms", flush=True)

    # ---- one host thread, from the downloaded placements ----
    f = pack_ref.IndexFile(path)
    os.unlink(path)
    lens = {(x[1], x[0]): x[3] - x[2] for x in f.bins}
    lut = np.full(256, 4, dtype=np.uint8)
    for k, c in enumerate(b"ACGT"):
        lut[c] = lut[c + 32] = k
    codes, ro = lut[np.asarray(bases, dtype=np.uint8)], np.asarray(off, dtype=np.int64)
    pick = np.sort(np.random.default_rng(1).choice(len(hits), size=min(args.host_hits, len(hits)), replace=False))
    t0 = time.perf_counter()
    table = host_table(pl[pick], ops, codes, ro, lens)
    host_ms = (time.perf_counter() - t0) * 1e3
    q = M.Pileup(0)
    with Stderr():
        q.add_run(ws, hits[pick], M.SLACK_ALL)
    same = all(np.array_equal(q.download(*key)[0], t) for key, t in table.items())
    scaled = host_ms / max(len(pick), 1) * len(hits)
    print(f"one host thread (numpy): {host_ms:.0f} ms for {len(pick)} placements, {scaled:.0f} ms scaled to all: "
          f"{scaled / (np.mean(steps['best']) + np.mean(steps['pile'])):.0f} times best + pile; counters identical: {same}", flush=True)
    q.close()
    p.close()
    ws.close()

    # ---- the deep pile ----
    rng = np.random.default_rng(7)
    seq = np.frombuffer(bytes(f.text[f.bins[3][2]:f.bins[3][3]]), dtype=np.uint8)
    start = 20000 + rng.integers(0, 151, size=args.deep_reads)
    deep = seq[start[:, None] + np.arange(READ_LEN)[None, :]].copy()
    sub = rng.random(deep.shape) < 0.01
    deep[sub] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(sub.sum()))]
    d_off = np.arange(args.deep_reads + 1, dtype=np.uint64) * READ_LEN
    ws = M.Batch(ix, 0, args.deep_reads, deep.size, lanes=1)
    ws.upload(deep.reshape(-1), d_off)
    ws.run()
    p = M.Pileup(0)
    steps, m = timed_add(p, ws, args.rounds)
    counts = p.download(f.bins[3][1], f.bins[3][0])[0]
    print(f"deep pile: {args.deep_reads} reads from one stretch of 300 bases, {m.group(1)} hits, {m.group(2)} piled; the deepest position holds "
          f"{int(counts[:, :7].sum(axis=1).max())}", flush=True)
    for s in ("best", "pile", "call"):
        print(f"  {s:10s} {spread(steps[s])} ms", flush=True)
    p.close()
    ws.close()
    if not same:
        sys.exit("pile_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
