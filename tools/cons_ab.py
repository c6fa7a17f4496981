#!/usr/bin/env python3
"""cons_ab.py -- what the consensus of a piled run costs on the device (k_cons.hip, mtsv_pileup_consensus), split into the call
pass, the layout and the write pass, beside one host thread that calls the same consensus from downloaded counters, and beside
a plain copy of the 33 bytes per slot that such a host thread needs first.

    timeout -k 10 500 python tools/cons_ab.py [--reads 1000000] [--rounds 5] [--host-refs 4]

The workload is binned, not made up: the synthetic index and reads of tools/pile_ab.py (64 taxa, 2 GIs each, 50,000 bases a
sequence; --reads reads of 150 bases from mtsv_synth_reads), run resident on one lane and piled once.

The device arm is mtsv_pileup_consensus under (min_depth 1, min_frac 0.5, min_breadth 0, fill N, width 60), --rounds times
after one warm-up call (which allocates), split by its own MTSV_PILE_TIMING line -- once with the plain write pass
(MTSV_CONS_WRITE=plain: byte stores), once with the staged one (staged: a tile's bytes through LDS, whole dwords stored) and
once as the library chooses; then the same with fasta == NULL (rows only: the call pass alone).  The host arm downloads the
counters of --host-refs references (mtsv_pileup_download), calls them with numpy on one thread, checks the text against the
device's for those references, and is scaled to all slots."""
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

READ_LEN = 150
CONS = re.compile(r"\[pile timing\] consensus segments (\d+) slots (\d+) tile (\d+) rows (\d+) bytes (\d+) write (\w+); call ([\d.]+) ms, layout ([\d.]+) ms, "
                  r"write ([\d.]+) ms, call_all ([\d.]+) ms")
PARAMS = (1, 500000, 0, 0, 60)


def timed(p, rounds, fasta):
    steps = {s: [] for s in ("call", "layout", "write", "call_all")}
    out = None
    for r in range(rounds + 1):                                # (call 0 allocates)
        with Stderr() as err:
            out = p.consensus(*PARAMS, fasta=fasta)
        m = CONS.search(err.text)
        if not m:
            sys.exit(f"cons_ab: no timing line in: {err.text!r}")
        if r:
            for s, x in zip(steps, m.groups()[6:]):
                steps[s].append(float(x))
    return steps, out, m


def host_consensus(counts, codes, width):
    """one host thread, numpy: the text of one reference's characters under PARAMS (without its header)"""
    n = counts[:-1, :7].astype(np.int64)
    ref = codes[:-1]
    depth = n.sum(axis=1)
    w = n.argmax(axis=1)                                       # (the first of equal counts: the lowest channel)
    top = n[np.arange(len(n)), w]
    fill = (depth < 1) | (w == 5) | (top * 1000000 < 500000 * depth)
    ch = np.where(w == 0, np.frombuffer(b"ACGTN", dtype=np.uint8)[np.minimum(ref, 4)], np.frombuffer(b"NACGTNN", dtype=np.uint8)[w])
    ch = np.where(fill, ord("N"), ch)
    ch = ch[fill | (w != 6)].astype(np.uint8).tobytes()
    return b"".join(ch[k:k + width] + b"\n" for k in range(0, len(ch), width))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-refs", type=int, default=4)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("cons_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_PILE_TIMING"] = "1"
    ix = M.MGIndex.synth(seed=5, n_taxa=64, gis_per_taxon=2, seq_len=50000)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=3, n_reads=args.reads, read_len=READ_LEN)
    ws = M.Batch(ix, 0, args.reads, len(bases), lanes=1)
    ws.upload(bases, off)
    ws.run()                                                   # (warms the clocks and the workspace)
    ws.run()
    texts = {}
    for form in ("plain", "staged", None):                     # the two write passes (read when an accumulator is created), then the default
        if form:
            os.environ["MTSV_CONS_WRITE"] = form
        else:
            os.environ.pop("MTSV_CONS_WRITE", None)
        p = M.Pileup(0)
        with Stderr():
            piled, skipped, _ = p.add_run(ws)
        info = p.info()
        if form == "plain":
            print(f"{args.reads} reads of {READ_LEN} bases, {piled} hits piled; {info['n_refs']} references, {info['n_slots']} slots, "
                  f"{info['device_bytes']} bytes on the device", flush=True)
        steps, (text, rows, _), m = timed(p, args.rounds, True)
        texts[form] = text
        print(f"consensus, write pass {m.group(6)}{'' if form else ' (the default)'}: {len(rows)} references, {len(text)} bytes of text "
              f"({len(text) / max(info['n_slots'], 1):.3f} per slot), tile {m.group(3)}", flush=True)
        for s in steps:
            print(f"  {s:10s} {spread(steps[s])} ms", flush=True)
        if form:
            p.close()
    if not texts["plain"] == texts["staged"] == texts[None]:
        sys.exit("cons_ab: the two write passes disagree")
    only, (_, rows_only, _), _ = timed(p, args.rounds, False)
    print(f"rows only: call {spread(only['call'])} ms, call_all {spread(only['call_all'])} ms; rows identical: {rows_only.tobytes() == rows.tobytes()}", flush=True)
    n_bytes = info["n_slots"] * 33
    print(f"hipMemcpyDtoD of 33 bytes per slot ({n_bytes} bytes): {dtod_ms(n_bytes):.3f} ms", flush=True)

    # ---- one host thread, from downloaded counters ----
    pieces = {}
    for piece in text.split(b">")[1:]:
        head, body = piece.split(b"\n", 1)
        pieces[head] = body
    pick = rows[:args.host_refs]
    t_down = t_call = 0.0
    slots, same = 0, True
    for r in pick:
        t0 = time.perf_counter()
        with Stderr():
            counts, codes = p.download(int(r["tax_id"]), int(r["gi"]))
        t1 = time.perf_counter()
        body = host_consensus(counts, codes, PARAMS[4])
        t2 = time.perf_counter()
        t_down, t_call, slots = t_down + (t1 - t0) * 1e3, t_call + (t2 - t1) * 1e3, slots + len(counts)
        same = same and body == pieces[b"%d-%d" % (int(r["gi"]), int(r["tax_id"]))]
    scale = info["n_slots"] / max(slots, 1)
    dev = np.mean(steps["call"]) + np.mean(steps["layout"]) + np.mean(steps["write"])
    print(f"one host thread (numpy): download {t_down:.1f} ms and call {t_call:.1f} ms for {len(pick)} references of {slots} slots; scaled to all "
          f"slots {t_down * scale:.0f} + {t_call * scale:.0f} ms: {(t_down + t_call) * scale / max(dev, 1e-9):.0f} times call + layout + write; "
          f"text identical: {same}", flush=True)
    p.close()
    ws.close()
    if not same:
        sys.exit("cons_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
