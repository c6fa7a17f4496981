#!/usr/bin/env python3
"""dedup_ab.py -- what binning identical reads once (k_dedup.hip, mtsv_batch_take_unique, mtsv_fold_expand) costs and saves,
beside the same run without it, inside one process on one device.

    timeout -k 10 900 python tools/dedup_ab.py [--reads 1048576] [--read-len 150] [--rates 0,0.3,0.7] [--steps 5] [--warmup 2] [--rounds 3]

A synthetic index (mtsv_synth_index) is made resident; a read set of --reads reads is sampled from it (mtsv_synth_reads), and
for every duplicate rate r that share of the reads is overwritten with copies of other reads of the set.  Two ways through a
step, in turn, --rounds times --steps steps each:

  (a) plain   mtsv_batch_upload, mtsv_batch_run, mtsv_fold_add_run
  (b) dedup   mtsv_batch_upload (intake), mtsv_batch_take_unique, mtsv_batch_run, mtsv_fold_add_run, mtsv_fold_expand

Both end with the same fold (checked once per rate, byte for byte).  Times are host clocks around calls that end in a device
synchronise.  The device times of hash, insert, resolve, scan, copy and of the expansion's two halves are those of the
library's own HIP events, read from the `[dedup]` and `[expand]` lines a map created under MTSV_TRACE prints, in steps of their
own after the timed rounds.  The row of rate 0 is what a caller who passes --dedup needlessly pays."""
import argparse
import contextlib
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mtsv_tools_amd as M  # noqa: E402


@contextlib.contextmanager
def stderr_to(path):
    """the process's stderr (the library's too) into a file while the block runs"""
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "ab") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)


def duplicated_rows(rows, rate, seed):
    """rows with a share `rate` of them overwritten by copies of rows that are not overwritten"""
    n = len(rows)
    rng = np.random.default_rng(seed)
    k = int(rate * n)
    if not k:
        return rows.copy()
    perm = rng.permutation(n)
    victims, keepers = perm[:k], perm[k:]
    out = rows.copy()
    out[victims] = rows[rng.choice(keepers, size=k)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--taxa", type=int, default=64)
    ap.add_argument("--seq-len", type=int, default=100000)
    ap.add_argument("--rates", default="0,0.3,0.7")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("dedup_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    n, L = args.reads, args.read_len
    ix = M.MGIndex.synth(seed=5, n_taxa=args.taxa, gis_per_taxon=2, seq_len=args.seq_len)
    ix.to_device(0)
    base_rows = np.asarray(M.synth_reads(ix, seed=1000, n_reads=n, read_len=L)[0]).reshape(n, L)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    print(f"synthetic index: {args.taxa} taxa x 2 GIs x {args.seq_len} bases; {n} reads of {L} bases per step; "
          f"{args.rounds} rounds x {args.steps} steps per way, {args.warmup} warm-up steps", flush=True)
    params = M.default_params()

    def workspace():
        b = M.Batch(ix, 0, n, n * L)
        b.set_assignments(M.ASSIGN_ONLY)
        return b

    plain, ws, intake = workspace(), workspace(), M.Batch(ix, 0, n, n * L, 1, lanes=1)
    f_plain, f_rep, f_all = M.Fold(0, M.GRAIN_TAXID, n), M.Fold(0, M.GRAIN_TAXID, n), M.Fold(0, M.GRAIN_TAXID)
    m = M.DupMap(0)
    os.environ["MTSV_TRACE"] = "1"
    traced = M.DupMap(0)
    del os.environ["MTSV_TRACE"]
    log = tempfile.NamedTemporaryFile(prefix="dedup_ab_", suffix=".log", delete=False).name
    table = []
    for rate in [float(x) for x in args.rates.split(",")]:
        pinned = M.HostBuffer(n * L)
        pinned.array.reshape(n, L)[:] = duplicated_rows(base_rows, rate, 7)
        bases = pinned.array

        def plain_step():
            t0 = time.perf_counter()
            plain.upload(bases, off)
            plain.run(params)
            t1 = time.perf_counter()
            f_plain.reset(n)
            f_plain.add_run(plain)
            t2 = time.perf_counter()
            return dict(step=(t2 - t0) * 1e3, run=(t1 - t0) * 1e3, fold=(t2 - t1) * 1e3)

        def dedup_step(dm=m):
            t0 = time.perf_counter()
            intake.upload(bases, off)
            n_unique, _, take_ms = ws.take_unique(intake, dm)
            t1 = time.perf_counter()
            ws.run(params)
            t2 = time.perf_counter()
            f_rep.reset(n)
            f_rep.add_run(ws)
            expand_ms = f_all.expand(f_rep, dm)
            t3 = time.perf_counter()
            return dict(step=(t3 - t0) * 1e3, take=(t1 - t0) * 1e3, run=(t2 - t1) * 1e3, fold=(t3 - t2) * 1e3, n_unique=n_unique, take_ms=take_ms,
                        expand_ms=expand_ms)

        plain_step()
        d = dedup_step()
        same = f_plain.download().tobytes() == f_all.download().tobytes()
        print(f"rate {rate:.2f}: {d['n_unique']} of {n} reads distinct; {f_plain.count()} records; folds of the two ways identical: {same}", flush=True)
        if not same:
            sys.exit("dedup_ab: the two ways disagree")
        ways = (("plain", plain_step), ("dedup", dedup_step))
        parts = {name: [] for name, _ in ways}
        for r in range(1, args.rounds + 1):
            for name, step in ways:
                for _ in range(args.warmup if r == 1 else 1):
                    step()
                each = [step() for _ in range(args.steps)]
                parts[name] += each
                print(f"  round {r} {name:5s} ms_per_step {np.mean([f['step'] for f in each]):9.3f}  steps: " + " ".join(f"{f['step']:.1f}" for f in each), flush=True)
        open(log, "wb").close()
        with stderr_to(log):
            for _ in range(args.steps):
                dedup_step(traced)
        text = open(log).read()
        k = {name: [float(x) for x in re.findall(r"\[dedup\].*?%s ([\d.]+) ms" % name, text)] for name in ("hash", "insert", "resolve", "scan", "copy")}
        k["count"] = [float(x) for x in re.findall(r"\[expand\].*count and scan ([\d.]+) ms", text)]
        k["write"] = [float(x) for x in re.findall(r"\[expand\].*write ([\d.]+) ms", text)]
        if any(len(v) != args.steps for v in k.values()):
            sys.exit("dedup_ab: the trace lines of the library were not found:\n" + text[-2000:])
        mean = lambda name, key: float(np.mean([f[key] for f in parts[name]]))  # noqa: E731
        lo = lambda name: min(f["step"] for f in parts[name])  # noqa: E731
        hi = lambda name: max(f["step"] for f in parts[name])  # noqa: E731
        km = {a: float(np.mean(v)) for a, v in k.items()}
        table.append((rate, d["n_unique"], km, mean("plain", "step"), lo("plain"), hi("plain"), mean("dedup", "step"), lo("dedup"), hi("dedup"),
                      mean("dedup", "take"), mean("plain", "run"), mean("dedup", "run")))
        pinned.close()
    print()
    print("| rate | distinct | hash | insert | resolve | scan | copy | expand count+scan | expand write | plain step (min..max) | dedup step (min..max) | upload+take | plain upload+run | dedup run |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for rate, nu, km, ps, pl, ph, ds, dl, dh, take, prun, drun in table:
        print(f"| {rate:.0%} | {nu} | {km['hash']:.3f} | {km['insert']:.3f} | {km['resolve']:.3f} | {km['scan']:.3f} | {km['copy']:.3f} | {km['count']:.3f} | "
              f"{km['write']:.3f} | {ps:.1f} ({pl:.1f}..{ph:.1f}) | {ds:.1f} ({dl:.1f}..{dh:.1f}) | {take:.1f} | {prun:.1f} | {drun:.1f} |")
    print("(device ms of the library's HIP events for the kernels; host ms around synchronous calls for the steps)")
    os.unlink(log)
    for x in (plain, ws, intake, f_plain, f_rep, f_all, m, traced):
        x.close()


if __name__ == "__main__":
    main()
