#!/usr/bin/env python3
"""collapse_ab.py -- mtsv-collapse on per-chunk result files without and with --on-gpu (k_parse.hip, mtsv_fold_add_text), and
where the device arm spends its time.

    timeout -k 10 900 python tools/collapse_ab.py [--files 4] [--reads 400000] [--rounds 3] [--modes taxid-gi,taxid] [FILE...]

Without FILEs the inputs are synthetic: one mtsv_synth_index database, --reads mtsv_synth_reads reads run once at
MTSV_GRAIN_LONG; file k of --files holds the long-format lines of a window of two (K + 1)-ths of the reads, so that
neighbouring files share half their reads, with every edit raised by k -- the fold has equal keys to join -- and with its
lines in the order of the run, which is not the order of the IDs.  With FILEs those are collapsed as they are.

Per mode the two arms alternate, --rounds times after one warm-up each, on one box: wall time of the process, outputs and
reports compared byte for byte.  The device arm is split by its own lines on stderr (MTSV_COLLAPSE_TIMING, MTSV_PARSE_TIMING,
MTSV_TEXT_TIMING = 1):
  host preparation   reading and splitting the files, the dictionary of IDs (one std::sort of all lines), cutting and staging
  upload             the text, offsets and reads of every mtsv_fold_add_text call
  parse kernels      k_parse count / tokens / heads / place / reduce and their two scans (device time)
  fold               k_fold count / scan / write (device time)
  text               the ID table and mtsv_fold_format_text (ID upload, k_text, copy of the text)
  report, write      mtsv_fold_taxa_report + formatting; the two files
  the rest           process start, HIP initialisation, allocation, the calls' host side
Beside the parse kernels: a hipMemcpyDtoD of the same hit bytes."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402

BIN = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
COLLAPSE = re.compile(r"\[collapse timing\] files (\d+) reads (\d+) calls (\d+) hit_bytes (\d+) tokens (\d+) text_bytes (\d+); read_split_dictionary ([0-9.]+) ms, "
                      r"staging ([0-9.]+) ms, add_text ([0-9.]+) ms, id_table_and_text ([0-9.]+) ms, report ([0-9.]+) ms, write ([0-9.]+) ms")
PARSE = re.compile(r"\[parse timing\] bytes \d+ lines \d+ tokens \d+ records (\d+); upload ([0-9.]+) ms, kernels ([0-9.]+) ms, fold ([0-9.]+) ms, call ([0-9.]+) ms")
TEXT = re.compile(r"\[text timing\] records (\d+) id_bytes (\d+) text_bytes (\d+); id_upload ([0-9.]+) ms, kernels ([0-9.]+) ms, text_copy ([0-9.]+) ms")


def synthetic_files(d, n_files, n_reads):
    M.set_build_device(0)
    ix = M.MGIndex.synth(4242, 64, 4, 50_000, threads=min(16, os.cpu_count() or 8))
    M.set_build_device(-1)
    ix.to_device(0)
    read_len = 150
    bases, off = M.synth_reads(ix, seed=77, n_reads=n_reads, read_len=read_len)
    b = M.Batch(ix, 0, n_reads, len(bases))
    b.set_assignment_grain(M.GRAIN_LONG)
    b.set_assignments(M.ASSIGN_ONLY)
    b.upload(bases, off)
    b.run()
    recs = b.download_assignments_gi()[0]
    b.close()
    ix.close()
    rng = np.random.default_rng(5)
    names = [f"read_{i:09d}/{int(x)}" for i, x in enumerate(rng.integers(0, 1 << 30, n_reads))]
    paths = []
    for k in range(n_files):
        lo, hi = k * n_reads // (n_files + 1), (k + 2) * n_reads // (n_files + 1)
        part = recs[(recs["read"] >= lo) & (recs["read"] < hi)].copy()
        part["edit"] += k
        text = M.format_assignments_gi(part, names)
        lines = text.splitlines(keepends=True)
        order = np.random.default_rng(100 + k).permutation(len(lines))      # (a run's order is not the IDs')
        p = os.path.join(d, f"chunk{k}.results")
        with open(p, "w") as f:
            f.write("".join(lines[i] for i in order))
        paths.append(p)
    return paths


def run(paths, mode, out, rep, on_gpu):
    env = dict(os.environ, MTSV_COLLAPSE_TIMING="1", MTSV_PARSE_TIMING="1", MTSV_TEXT_TIMING="1")
    t0 = time.perf_counter()
    r = subprocess.run([BIN, "-o", out, "--report", rep, "--mode", mode, *(["--on-gpu", "-v"] if on_gpu else []), *paths], capture_output=True, text=True, env=env)
    wall = (time.perf_counter() - t0) * 1e3
    if r.returncode != 0:
        raise SystemExit(f"collapse_ab: mtsv-collapse {'--on-gpu ' if on_gpu else ''}failed with {r.returncode}: {r.stderr[-600:]}")
    return wall, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--reads", type=int, default=400_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="taxid-gi,taxid")
    ap.add_argument("paths", nargs="*")
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("collapse_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    with tempfile.TemporaryDirectory() as d:
        paths = args.paths or synthetic_files(d, args.files, args.reads)
        size = sum(os.path.getsize(p) for p in paths)
        print(f"{len(paths)} files, {size} bytes" + ("" if args.paths else f" (synthetic: {args.reads} reads, neighbouring files share half their reads)"), flush=True)
        for mode in args.modes.split(","):
            outs = {arm: (os.path.join(d, f"{arm}.txt"), os.path.join(d, f"{arm}.tsv")) for arm in ("host", "device")}
            walls = {"host": [], "device": []}
            splits = []
            for r in range(args.rounds + 1):  # (round 0 warms up: the page cache, the code objects)
                for arm in ("host", "device"):
                    wall, err = run(paths, mode, *outs[arm], on_gpu=arm == "device")
                    if arm == "device":
                        if "the host path takes the input" in err:
                            raise SystemExit(f"collapse_ab: {mode}: the device arm fell back to the host path: {err[-400:]}")
                        c, t = COLLAPSE.search(err), TEXT.search(err)
                        p = [tuple(float(x) for x in m) for m in PARSE.findall(err)]
                        if not c or not t or not p:
                            raise SystemExit("collapse_ab: the timing lines are missing: " + err[-600:])
                        cg = [float(x) for x in c.groups()]
                        pa = np.array(p)
                        splits.append(dict(prep=cg[6] + cg[7], add=cg[8], upload=pa[:, 1].sum(), parse=pa[:, 2].sum(), fold=pa[:, 3].sum(), text=cg[9],
                                           id_upload=float(t.group(4)), k_text=float(t.group(5)), text_copy=float(t.group(6)), report=cg[10], write=cg[11],
                                           calls=cg[2], hit_bytes=cg[3], tokens=cg[4], text_bytes=cg[5], reads=cg[1], records=pa[:, 0].sum(), dict_ms=cg[6], staging=cg[7]))
                    if r:
                        walls[arm].append(wall)
                    print(f"{mode:9s} round {r} arm {arm:6s} wall {wall:9.1f} ms" + (" (warm-up)" if not r else ""), flush=True)
            same = all(open(outs["host"][k], "rb").read() == open(outs["device"][k], "rb").read() for k in (0, 1))
            print(f"{mode}: output and report of the two arms are the same bytes: {same}", flush=True)
            if not same:
                raise SystemExit("collapse_ab: the arms differ")
            s = {k: float(np.mean([x[k] for x in splits[1:]])) for k in splits[0]}
            hm, dm = float(np.mean(walls["host"])), float(np.mean(walls["device"]))
            spread = max(walls["host"]) - min(walls["host"])
            known = s["prep"] + s["add"] + s["text"] + s["report"] + s["write"]
            print(f"{mode} host  : {hm:9.1f} ms (rounds {min(walls['host']):.1f}..{max(walls['host']):.1f})", flush=True)
            print(f"{mode} device: {dm:9.1f} ms (rounds {min(walls['device']):.1f}..{max(walls['device']):.1f}); {int(s['reads'])} IDs, {int(s['calls'])} calls, "
                  f"{int(s['hit_bytes'])} hit bytes, {int(s['tokens'])} tokens, {int(s['records'])} records in, {int(s['text_bytes'])} bytes out", flush=True)
            print(f"{mode} device split: host preparation {s['prep']:.1f} ms (read + split + dictionary {s['dict_ms']:.1f}, cut + staging {s['staging']:.1f}); "
                  f"add_text calls {s['add']:.1f} ms of which upload {s['upload']:.2f}, parse kernels {s['parse']:.3f}, fold kernels {s['fold']:.3f}; "
                  f"ID table + text {s['text']:.1f} ms of which ID upload {s['id_upload']:.2f}, k_text {s['k_text']:.3f}, copy {s['text_copy']:.2f}; "
                  f"report {s['report']:.1f} ms; write {s['write']:.1f} ms; the rest (process start, HIP initialisation, allocation) {dm - known:.1f} ms", flush=True)
            print(f"{mode}: parse kernels {s['parse']:.3f} ms for {int(s['hit_bytes'])} hit bytes; hipMemcpyDtoD of as many bytes {dtod_ms(int(s['hit_bytes'])):.3f} ms", flush=True)
            print(f"{mode}: device minus host = {dm - hm:+.1f} ms; the host arm's spread between rounds is {spread:.1f} ms "
                  f"({'beyond' if abs(dm - hm) > spread else 'within'} the spread)", flush=True)


if __name__ == "__main__":
    main()
