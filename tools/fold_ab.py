#!/usr/bin/env python3
"""fold_ab.py -- what folding chunk runs into an accumulator of records (k_fold.hip, mtsv_fold_add_run, mtsv-binner
--fold-on-gpu) costs, and where a run that keeps ONE chunk resident at a time spends its time.

    timeout -k 10 1100 python tools/fold_ab.py [--chunks 8] [--reads N] [--block-reads 1048576] [--rounds 3] [--cli-reads 2000000] [--cli-runs 3]

The workload is that of `bench.py --mode chunks` (BASELINE config 5) on one GPU: --chunks synthetic database chunks
(bench.py's index files, built and written when they are not there) and reads sampled from every chunk in equal shares.

Part 1, in this process, --rounds times: the chunks take turns -- mtsv_index_load, mtsv_index_to_device, one workspace in
MTSV_ASSIGN_ONLY, per block of --block-reads reads upload + run + mtsv_fold_add_run into the block's fold, workspace and index
closed.  Per chunk: the fold's device_ms (summed over the blocks) beside a hipMemcpyDtoD that moves the same bytes (what the
folds read, accumulator and run, plus what they write: a copy of half that sum reads and writes as much), and beside the
chunk's runs (stage_ms[7], summed over the blocks); the host time of loading the chunk and of making it resident.

Part 2, the command line, --cli-runs times each on --cli-reads reads in a FASTQ file: mtsv-binner --merge-on-gpu (every chunk
resident) against --fold-on-gpu (one at a time), wall time of the process, the files compared byte for byte, and the share of
the folded run spent in mtsv_index_load and mtsv_index_to_device (its MTSV_CLI_TIMING line)."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402
from merge_ab import CHUNK_SPEC, load_chunks  # noqa: E402

BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def chunk_path(c, n_chunks):
    return f"/tmp/mtsv_bench_config5_c{c}of{n_chunks}.idx"


def spread(v):
    return f"{np.mean(v):.3f} (min {min(v):.3f}, max {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--block-reads", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cli-reads", type=int, default=2_000_000)
    ap.add_argument("--cli-runs", type=int, default=3)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("fold_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    n_reads, read_len = args.reads or CHUNK_SPEC[3], CHUNK_SPEC[4]
    K = args.chunks
    chunks = load_chunks(K)  # (builds and writes the files when they are missing; all resident for the reads' sampling)
    share = [n_reads // K + (1 if c < n_reads % K else 0) for c in range(K)]
    pinned = M.HostBuffer(n_reads * read_len)
    at = 0
    for c in range(K):
        part, _ = M.synth_reads(chunks[c], seed=2000 + c, n_reads=share[c], read_len=read_len)
        pinned.array[at:at + len(part)] = part
        at += len(part)
    for ix in chunks:
        ix.close()  # from here on one chunk at a time
    bases = pinned.array
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    params = M.default_params()
    B = min(args.block_reads, n_reads)
    blocks = [(a, min(n_reads, a + B)) for a in range(0, n_reads, B)]
    print(f"{K} chunks, one resident at a time; {n_reads} reads of {read_len} bases in {len(blocks)} blocks of {B}", flush=True)

    # ---- part 1 ----
    folds = [M.Fold(0, M.GRAIN_TAXID) for _ in blocks]
    rec = M.ASSIGN_DTYPE.itemsize
    per_chunk = [dict(fold=[], run=[], load=[], resident=[], traffic=0, n_b=0) for _ in range(K)]
    totals, run_records = [], {}
    for r in range(args.rounds + 1):  # (round 0 warms up: code objects, the pool)
        for (a, b), f in zip(blocks, folds):
            f.reset(b - a)
        t_round = time.perf_counter()
        for c in range(K):
            t0 = time.perf_counter()
            ix = M.MGIndex.load(chunk_path(c, K))
            t1 = time.perf_counter()
            ix.to_device(0)
            t2 = time.perf_counter()
            ws = M.Batch(ix, 0, B, B * read_len, lanes=1)
            ws.set_assignments(M.ASSIGN_ONLY)
            fold_ms = run_ms = 0.0
            traffic = n_b = 0
            for k, ((a, b), f) in enumerate(zip(blocks, folds)):
                ws.upload(bases[a * read_len:b * read_len], off[a:b + 1] - off[a])
                ws.run(params)
                run_ms += ws.stats()["stage_ms"]["total"]
                before = f.count()
                fold_ms += f.add_run(ws)
                if r == 0:  # (the run's record count, once: the warm-up round is not timed)
                    run_records[c, k] = len(ws.download_assignments()[0])
                traffic += (before + run_records[c, k] + f.count()) * rec
                n_b += run_records[c, k]
            ws.close()
            ix.close()
            if r:
                pc = per_chunk[c]
                pc["fold"].append(fold_ms)
                pc["run"].append(run_ms)
                pc["load"].append((t1 - t0) * 1e3)
                pc["resident"].append((t2 - t1) * 1e3)
                pc["traffic"], pc["n_b"] = traffic, n_b
        if r:
            totals.append((time.perf_counter() - t_round) * 1e3)
    n_final = sum(f.count() for f in folds)
    print(f"accumulated records after the last chunk: {n_final} ({n_final * rec} bytes in {len(folds)} folds)", flush=True)
    for c in range(K):
        pc = per_chunk[c]
        copy_ms = dtod_ms(max(pc["traffic"] // 2, 1))
        print(f"chunk {c}: fold device_ms {spread(pc['fold'])} for {pc['n_b']} run records, {pc['traffic']} bytes read + written; hipMemcpyDtoD moving the same bytes "
              f"{copy_ms:.3f} ms: the fold takes {np.mean(pc['fold']) / copy_ms:.2f} times the copy; the chunk's runs (stage_ms[7]) {spread(pc['run'])} ms: the fold is "
              f"{100 * np.mean(pc['fold']) / np.mean(pc['run']):.2f} % of them; mtsv_index_load {spread(pc['load'])} ms, mtsv_index_to_device {spread(pc['resident'])} ms", flush=True)
    s = {k: sum(np.mean(pc[k]) for pc in per_chunk) for k in ("fold", "run", "load", "resident")}
    print(f"all chunks: {spread(totals)} ms per pass over the chunks; of it folds {s['fold']:.3f} ms (device), runs {s['run']:.3f} ms (device), "
          f"mtsv_index_load {s['load']:.3f} ms, mtsv_index_to_device {s['resident']:.3f} ms: loading and making resident are "
          f"{100 * (s['load'] + s['resident']) / np.mean(totals):.1f} % of a pass", flush=True)
    for f in folds:
        f.close()

    # ---- part 2 ----
    if args.cli_runs > 0 and args.cli_reads > 0:
        n_cli = min(args.cli_reads, n_reads)
        d = f"/tmp/mtsv_fold_ab_{os.getpid()}"
        os.makedirs(d, exist_ok=True)
        fq = os.path.join(d, "reads.fastq")
        step = n_reads // n_cli  # (every chunk's share is represented)
        rows = np.asarray(bases).reshape(n_reads, read_len)[::step][:n_cli]
        qual = b"I" * read_len
        with open(fq, "wb") as fh:
            for i, row in enumerate(rows):
                fh.write(b"@r%d\n" % i + row.tobytes() + b"\n+\n" + qual + b"\n")
        index = ",".join(chunk_path(c, K) for c in range(K))
        wall = {"--merge-on-gpu": [], "--fold-on-gpu": []}
        shares = []
        for k in range(args.cli_runs + 1):  # (run 0 warms the page cache)
            for switch in wall:
                tag = switch.strip("-").split("-")[0]
                out = [os.path.join(d, f"{tag}.{x}") for x in ("res", "rep", "m", "u")]
                t0 = time.perf_counter()
                p = subprocess.run([BINNER, "--fastq", fq, "-i", index, "-m", out[0], "--force-overwrite", switch, "--report", out[1], "--matched", out[2],
                                    "--unmatched", out[3]], capture_output=True, text=True, env={**os.environ, "MTSV_CLI_TIMING": "1"})
                dt = time.perf_counter() - t0
                if p.returncode != 0:
                    sys.exit(f"fold_ab: mtsv-binner {switch} failed:\n{p.stdout}{p.stderr}")
                if k:
                    wall[switch].append(dt * 1e3)
                m = re.search(r"index_load ([\d.]+) s, index_to_device ([\d.]+) s, upload_and_run ([\d.]+) s, fold ([\d.]+) s \(device ([\d.]+) ms\)", p.stderr)
                if k and switch == "--fold-on-gpu" and m:
                    shares.append([float(x) for x in m.groups()])
        same = all(open(os.path.join(d, f"merge.{x}"), "rb").read() == open(os.path.join(d, f"fold.{x}"), "rb").read() for x in ("res", "rep", "m", "u"))
        print(f"command line on {n_cli} reads, {K} chunks: files of the two switches identical: {same}", flush=True)
        for switch, v in wall.items():
            print(f"mtsv-binner {switch}: {spread(v)} ms per process", flush=True)
        if shares:
            sh = np.mean(np.array(shares), axis=0)
            w = np.mean(wall["--fold-on-gpu"]) / 1e3
            print(f"--fold-on-gpu: mtsv_index_load {sh[0]:.3f} s, mtsv_index_to_device {sh[1]:.3f} s ({100 * (sh[0] + sh[1]) / w:.1f} % of the process together), "
                  f"upload and run {sh[2]:.3f} s, fold {sh[3]:.3f} s of host time ({sh[4]:.3f} ms of device time)", flush=True)
        for name in os.listdir(d):
            os.remove(os.path.join(d, name))
        os.rmdir(d)
        if not same:
            sys.exit("fold_ab: --fold-on-gpu and --merge-on-gpu disagree")
    pinned.close()


if __name__ == "__main__":
    main()
