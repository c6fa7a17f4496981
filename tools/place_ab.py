#!/usr/bin/env python3
"""place_ab.py -- what the alignments of a run's hits cost on the device (k_place.hip, mtsv_batch_place_hits), beside the
verify stage of the run that produced the hits, beside a plain copy of the ring bytes the kernel wrote, and beside one host
thread doing the same from downloaded hits.

    timeout -k 10 500 python tools/place_ab.py [--reads 1000000] [--rounds 5] [--host-hits 2000]

The workload is binned, not made up: a synthetic index (64 taxa, 2 GIs each, 50,000 bases a sequence) and --reads reads of
150 bases from mtsv_synth_reads (one in ten random, the rest with the noise that call adds) -- the read length and noise of
the benchmark's config2 on a small index -- run resident on one lane.

The device arm is mtsv_batch_place_hits(hits = NULL), --rounds times after one warm-up (which allocates and warms the clocks),
split by its own MTSV_PLACE_TIMING line into scan (the map pass and the scan of the op slots), kernel and download.  Beside
it: stage_ms[verify] and the total of the run whose hits are placed; hipMemcpyDtoD of as many bytes as the kernel stored into
its ring; and one host thread placing --host-hits of the downloaded hits by the restatement of the tests (tests/place_ref.py:
the whole matrix by numpy columns, a traceback), compared with the device's placements and scaled to all hits."""
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
import place_ref  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402
from lca_ab import Stderr, spread  # noqa: E402

READ_LEN = 150
LINE = re.compile(r"\[place timing\] hits (\d+) slots (\d+) words (\d+) ring_cols (\d+) blocks (\d+) ring_bytes (\d+); scan ([\d.]+) ms, kernel ([\d.]+) ms, "
                  r"download ([\d.]+) ms, call ([\d.]+) ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-hits", type=int, default=2000)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("place_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_PLACE_TIMING"] = "1"
    ix = M.MGIndex.synth(seed=5, n_taxa=64, gis_per_taxon=2, seq_len=50000)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"place_ab_{os.getpid()}.idx")
    ix.write(path)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=3, n_reads=args.reads, read_len=READ_LEN)
    ws = M.Batch(ix, 0, args.reads, len(bases), lanes=1)
    ws.upload(bases, off)
    ws.run()                                                  # (warms the clocks and the workspace)
    ws.run()
    st = ws.stats()
    verify, total = st["stage_ms"]["verify"], st["stage_ms"]["total"]
    hits = ws.download()
    print(f"{args.reads} reads of {READ_LEN} bases, {len(hits)} hits; the run: verify {verify:.3f} ms of {total:.3f} ms", flush=True)

    steps = {s: [] for s in ("scan", "kernel", "download", "call")}
    pl = ops = m = None
    for r in range(args.rounds + 1):                          # (call 0 builds the table and allocates)
        with Stderr() as err:
            pl, ops, _ = ws.place_hits()
        m = LINE.search(err.text)
        if not m:
            sys.exit(f"place_ab: no timing line in: {err.text!r}")
        if r:
            for s, x in zip(steps, m.groups()[6:]):
                steps[s].append(float(x))
    ring_bytes = int(m.group(6))
    print(f"{m.group(1)} hits, {m.group(2)} op slots, {m.group(3)} words a column, a ring of {m.group(4)} columns, {m.group(5)} workgroups; "
          f"{ring_bytes} ring bytes stored ({ring_bytes / max(len(hits), 1):.0f} a hit), {int(pl['n_ops'].sum())} ops written", flush=True)
    for s in steps:
        print(f"  {s:8s} {spread(steps[s])} ms", flush=True)
    device = [a + b for a, b in zip(steps["scan"], steps["kernel"])]
    print(f"device: scan + kernel {spread(device)} ms = {np.mean(device) / verify:.2f} of the run's verify stage, {np.mean(device) / total:.2f} of the run", flush=True)
    copy_ms = dtod_ms(ring_bytes)
    print(f"hipMemcpyDtoD of the {ring_bytes} ring bytes: {copy_ms:.3f} ms: the kernel takes {np.mean(steps['kernel']) / copy_ms:.2f} times the copy", flush=True)

    # ---- one host thread, from the downloaded hits ----
    f = pack_ref.IndexFile(path)
    os.unlink(path)
    text_of = {(x[1], x[0]): bytes(f.text[x[2]:x[3]]) for x in f.bins}
    pick = np.random.default_rng(1).choice(len(hits), size=min(args.host_hits, len(hits)), replace=False)
    raw, ro = np.asarray(bases, dtype=np.uint8).tobytes(), np.asarray(off, dtype=np.int64)
    t0 = time.perf_counter()
    want = [place_ref.place_hit(raw[ro[int(h["read"])]:ro[int(h["read"]) + 1]], int(h["strand"]), text_of[(int(h["tax_id"]), int(h["gi"]))],
                                int(h["offset"]), int(h["edit"])) for h in hits[pick]]
    host_ms = (time.perf_counter() - t0) * 1e3
    same = all(w is not None and (int(p["ref_start"]), int(p["ref_end"]), ops[int(p["ops_off"]):int(p["ops_off"]) + int(p["n_ops"])].tolist())
               == (w[0], w[1], place_ref.encode(w[2])) for p, w in zip(pl[pick], want))
    scaled = host_ms / max(len(pick), 1) * len(hits)
    print(f"one host thread (numpy, tests/place_ref.py): {host_ms:.0f} ms for {len(pick)} hits, {scaled:.0f} ms scaled to all: {scaled / np.mean(steps['call']):.0f} times "
          f"the device call; placements identical: {same}", flush=True)
    ws.close()
    if not same:
        sys.exit("place_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
