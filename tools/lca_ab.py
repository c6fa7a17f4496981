#!/usr/bin/env python3
"""lca_ab.py -- what the per-read LCA and the clade rows cost on the device (k_lca.hip, mtsv_fold_lca), beside one host thread
doing the same from downloaded records and beside a plain copy of the record bytes.

    timeout -k 10 500 python tools/lca_ab.py [--reads 4000000] [--species 16384] [--rounds 5] [--slack 0]

The workload is synthetic: a taxonomy of --species species, 16 to a genus, 16 genera to a family, 16 families to an order, the
orders under one root; --reads reads of 1 to 8 records each (2.9 on average), the TaxIDs of a read in one genus -- or, for
one read in eight, anywhere -- with edits 0 to 3.  The records go into a fold through mtsv_fold_add_records.

The device arm is mtsv_fold_lca with an output fold and the rows, --rounds times after one warm-up, split by its own
MTSV_LCA_TIMING line into tree build (the first call only: later calls find the union and the taxonomy unchanged), the five
kernel steps (heads and scan, segmented minimum, segmented span, walk, scan and clade) and the download of the counters and
the nodes' counts.  Arm (a): numpy on one thread over the downloaded records -- segment minima, filter, node spans, the walk,
the prefix sums -- its result compared with the device's, records and rows.  Arm (b): hipMemcpyDtoD of the record bytes."""
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

SPECIES0, GENUS0, FAMILY0, ORDER0, TOP = 1_000_000, 500_000, 100_000, 10_000, 1


def spread(v):
    return f"{np.mean(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"


def parents_of(n_species):
    """{tax: parent} of the synthetic taxonomy"""
    par = {TOP: TOP}
    for s in range(n_species):
        par[SPECIES0 + s] = GENUS0 + s // 16
        par[GENUS0 + s // 16] = FAMILY0 + s // 256
        par[FAMILY0 + s // 256] = ORDER0 + s // 4096
        par[ORDER0 + s // 4096] = TOP
    return par


def make_records(n_reads, n_species, seed=1):
    rng = np.random.default_rng(seed)
    count = rng.choice(np.arange(1, 9), size=n_reads, p=[0.35, 0.2, 0.15, 0.1, 0.08, 0.06, 0.04, 0.02])
    read = np.repeat(np.arange(n_reads, dtype=np.uint64), count)
    j = np.arange(len(read)) - np.repeat(np.cumsum(count) - count, count)
    base = np.repeat(rng.integers(0, n_species, size=n_reads), count)
    wide = np.repeat(rng.random(n_reads) < 0.125, count)
    # in one genus: the genus's 16 species from a start on, distinct for up to 16 records; anywhere: strides of 4099 species
    species = np.where(wide, (base + j * 4099) % n_species, (base // 16) * 16 + (base + j) % 16)
    a = np.zeros(len(read), dtype=M.ASSIGN_DTYPE)
    a["read"], a["tax_id"], a["edit"] = read, SPECIES0 + species, rng.integers(0, 4, size=len(read))
    a = a[np.lexsort((a["tax_id"], a["read"]))]
    keep = np.ones(len(a), dtype=bool)
    keep[1:] = (a["read"][1:] != a["read"][:-1]) | (a["tax_id"][1:] != a["tax_id"][:-1])  # (keys must be distinct)
    return a[keep]


def host_lca(rec, par, slack):
    """numpy on one thread: (per-read records, {tax: (direct, clade)})"""
    # the tree in preorder, children ascending: an explicit stack
    kids = {}
    for t, p in par.items():
        if t != p:
            kids.setdefault(p, []).append(t)
    order, parent_no, stack = [0], [0], [(t, 0) for t in sorted((t for t, p in par.items() if t == p), reverse=True)]
    while stack:
        t, pn = stack.pop()
        me = len(order)
        order.append(t)
        parent_no.append(pn)
        stack.extend((k, me) for k in sorted(kids.get(t, []), reverse=True))
    order, parent_no = np.array(order, dtype=np.int64), np.array(parent_no, dtype=np.int64)
    last = np.arange(len(order))
    for i in range(len(order) - 1, 0, -1):
        last[parent_no[i]] = max(last[parent_no[i]], last[i])
    by_tax = np.argsort(order)
    node = by_tax[np.searchsorted(order[by_tax], rec["tax_id"].astype(np.int64))]
    head = np.ones(len(rec), dtype=bool)
    head[1:] = rec["read"][1:] != rec["read"][:-1]
    start = np.flatnonzero(head)
    seg = np.cumsum(head) - 1
    edit = rec["edit"].astype(np.int64)
    m = np.minimum.reduceat(edit, start)
    enters = edit <= np.minimum(m[seg] + slack, 0xffffffff)
    lo = np.minimum.reduceat(np.where(enters, node, len(order)), start)
    hi = np.maximum.reduceat(np.where(enters, node, -1), start)
    a = lo.copy()
    while True:
        up = last[a] < hi
        if not up.any():
            break
        a[up] = parent_no[a[up]]
    out = np.zeros(len(start), dtype=M.ASSIGN_DTYPE)
    out["read"], out["tax_id"], out["edit"] = rec["read"][start], order[a], m
    direct = np.bincount(a, minlength=len(order))
    prefix = np.concatenate(([0], np.cumsum(direct)))
    clade = prefix[last + 1] - prefix[:-1]
    return out, {int(order[i]): (int(direct[i]), int(clade[i])) for i in np.flatnonzero(clade)}


class Stderr:
    """what the library writes to stderr while the block runs"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


STEPS = ("tree", "heads", "min", "span", "walk", "clade", "download", "call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--species", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slack", type=int, default=0)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("lca_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_LCA_TIMING"] = "1"
    par = parents_of(args.species)
    with tempfile.NamedTemporaryFile("w", suffix=".dmp", delete=False) as fh:
        fh.write("".join(f"{t}\t|\t{p}\t|\trank{len(str(t))}\t|\n" for t, p in par.items()))
    t0 = time.perf_counter()
    tx = M.Taxonomy(fh.name)
    load_ms = (time.perf_counter() - t0) * 1e3
    os.remove(fh.name)
    rec = make_records(args.reads, args.species)
    n_bytes = len(rec) * M.ASSIGN_DTYPE.itemsize
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=args.reads)
    fold.add_records(rec)
    out = M.Fold(0, M.GRAIN_TAXID)
    print(f"{len(rec)} records ({n_bytes} bytes) of {len(np.unique(rec['read']))} reads; taxonomy of {len(par)} nodes loaded in {load_ms:.3f} ms; slack {args.slack}", flush=True)

    times = {s: [] for s in STEPS}
    first = None
    for r in range(args.rounds + 1):  # (call 0 builds the tree and warms up)
        with Stderr() as err:
            rows, total, ms = fold.lca(tx, args.slack, out=out)
        m = re.search(r"\[lca timing\] records (\d+) reads (\d+) nodes (\d+) taxa (\d+) rebuilt (\d); " + ", ".join(f"{s} ([\\d.]+) ms" for s in STEPS), err.text)
        if not m:
            sys.exit(f"lca_ab: no timing line in: {err.text!r}")
        v = [float(x) for x in m.groups()[5:]]
        if r == 0:
            first = (m.groups(), v)
        else:
            if m.group(5) != "0":
                sys.exit("lca_ab: the tree was rebuilt with the union and the taxonomy unchanged")
            for s, x in zip(STEPS, v):
                times[s].append(x)
    g = first[0]
    print(f"device tree: {g[2]} nodes for {g[3]} TaxIDs, built and uploaded in {first[1][0]:.3f} ms by the first call; later calls: {spread(times['tree'])} ms", flush=True)
    kernels = [sum(times[s][k] for s in STEPS[1:6]) for k in range(args.rounds)]
    for s in STEPS[1:7]:
        print(f"  {s:8s} {spread(times[s])} ms", flush=True)
    print(f"device: kernels {spread(kernels)} ms, whole call {spread(times['call'])} ms", flush=True)
    copy_ms = dtod_ms(n_bytes)
    print(f"(b) hipMemcpyDtoD of the {n_bytes} record bytes: {copy_ms:.3f} ms: the kernels take {np.mean(kernels) / copy_ms:.2f} times the copy", flush=True)

    # ---- arm (a): one host thread, from the downloaded records ----
    host = []
    for r in range(min(args.rounds, 3)):
        t0 = time.perf_counter()
        down = fold.download()
        t1 = time.perf_counter()
        want, clades = host_lca(down, par, args.slack)
        host.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    got = out.download()
    same = got.tobytes() == want.tobytes() and total == len(want) and {int(r["tax_id"]): (int(r["direct"]), int(r["clade"])) for r in rows} == clades
    both = [a + b for a, b in host]
    print(f"(a) one host thread: download {spread([a for a, _ in host])} ms, numpy {spread([b for _, b in host])} ms: {np.mean(both) / np.mean(times['call']):.1f} times "
          f"the device call, {np.mean(both) / np.mean(kernels):.1f} times its kernels; records and rows identical: {same}", flush=True)
    for f in (fold, out):
        f.close()
    if not same:
        sys.exit("lca_ab: the host thread and the device disagree")


if __name__ == "__main__":
    main()
