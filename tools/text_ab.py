#!/usr/bin/env python3
"""text_ab.py -- what writing the result lines on the device (k_text.hip, mtsv_batch_format_text) gains or costs against one
host thread, measured through the library.

    python tools/text_ab.py [--workload config2] [--steps 5] [--warmup 2] [--rounds 3] [--grains taxid,long,taxid-gi] [--reads N]

The same index file and reads as bench.py.  Per grain the reads are uploaded and run once in MTSV_ASSIGN_ONLY; the run's
records stay in HBM and both arms make the result text of that run from them, --rounds times --steps steps each, the arms
alternating within one process on one box:
  (a) host    mtsv_batch_download_assignments(_gi), then mtsv_format_assignments(_gi) on the calling thread
  (b) device  mtsv_batch_format_text: the IDs go up, measure + scan + write run, the text comes down
Both arms end with the same bytes on the host (checked once per grain).  Printed: every round's mean and every step; per arm
the time per step and per 10 M reads; for (a) its two parts; for (b) the library's own split of a call (MTSV_TEXT_TIMING=1:
ID upload, kernels -- the call's device_ms --, copy of the text) as means over the timed steps; the bytes that cross to the
host in each arm (records against text) and up to the device in (b) (the ID table); and the spread of arm (a) between its
rounds.  A difference between the arms counts only beyond that spread."""
import argparse
import ctypes
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
from mtsv_tools_amd import _lib as L  # noqa: E402
from report_ab import load_index  # noqa: E402  (bench.py's index file, built and written when it is not there)

GRAINS = {"taxid": M.GRAIN_TAXID, "taxid-gi": M.GRAIN_TAXID_GI, "long": M.GRAIN_LONG}
LINE = re.compile(r"\[text timing\] records (\d+) id_bytes (\d+) text_bytes (\d+); id_upload ([0-9.]+) ms, kernels ([0-9.]+) ms, text_copy ([0-9.]+) ms")


def with_stderr(fn):
    """fn() with stderr caught: (its result, the text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--grains", default="taxid,long,taxid-gi")
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("text_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    os.environ["MTSV_TEXT_TIMING"] = "1"  # (read when a workspace's formatter is created)
    ix, n_reads, read_len, desc = load_index(args.workload)
    if args.reads:
        n_reads = args.reads
    bases, off = M.synth_reads(ix, seed=1000, n_reads=n_reads, read_len=read_len)
    print(f"{args.workload}: {desc}; {n_reads} reads per step", flush=True)
    ids_blob = b"".join(b"r%d\0" % i for i in range(n_reads))
    id_off = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum([len(b"r%d" % i) + 1 for i in range(n_reads)], out=id_off[1:])
    per_10m = 1e7 / n_reads
    lib = M.lib()

    for gname in args.grains.split(","):
        grain = GRAINS[gname]
        wide = grain != M.GRAIN_TAXID
        rec_bytes = 24 if wide else 16
        b = M.Batch(ix, 0, n_reads, len(bases))
        b.set_assignment_grain(grain)
        b.set_assignments(M.ASSIGN_ONLY)
        b.upload(bases, off)
        b.run()

        def host_step(keep=False):
            """(ms download, ms format, bytes to the host, the text when asked for)"""
            a_p, a_n, a_ms = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_float()
            out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
            get = lib.mtsv_batch_download_assignments_gi if wide else lib.mtsv_batch_download_assignments
            fmt = lib.mtsv_format_assignments_gi if wide else lib.mtsv_format_assignments
            t0 = time.perf_counter()
            L._check(get(b.h, ctypes.byref(a_p), ctypes.byref(a_n), ctypes.byref(a_ms)))
            t1 = time.perf_counter()
            L._check(fmt(a_p, a_n.value, ids_blob, id_off.ctypes.data, n_reads, ctypes.byref(out_p), ctypes.byref(out_n)))
            t2 = time.perf_counter()
            text = ctypes.string_at(out_p.value, out_n.value) if keep else None
            lib.mtsv_free(a_p)
            lib.mtsv_free(out_p)
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, a_n.value * rec_bytes, text

        def device_step(keep=False):
            """(ms of the call, the library's split, bytes to the host, the text when asked for)"""
            out_p, out_n, ms = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_float()

            def call():
                t0 = time.perf_counter()
                L._check(lib.mtsv_batch_format_text(b.h, ids_blob, id_off.ctypes.data, n_reads, ctypes.byref(out_p), ctypes.byref(out_n), ctypes.byref(ms)))
                return (time.perf_counter() - t0) * 1e3

            wall, err = with_stderr(call)
            m = LINE.search(err)
            if not m:
                raise SystemExit("text_ab: the library printed no [text timing] line: " + err[-400:])
            text = ctypes.string_at(out_p.value, out_n.value) if keep else None
            lib.mtsv_free(out_p)
            return wall, tuple(float(x) for x in m.groups()[3:]), out_n.value, int(m.group(2)), text

        same = host_step(True)[3] == device_step(True)[4]
        print(f"{gname}: both arms give the same bytes: {same}", flush=True)
        if not same:
            raise SystemExit("text_ab: the arms differ")
        means = {"host": [], "device": []}
        parts = {"host": [], "device": []}
        to_host = {}
        up = 0
        for r in range(1, args.rounds + 1):
            for arm in ("host", "device"):
                for _ in range(args.warmup if r == 1 else 1):
                    (host_step if arm == "host" else device_step)()
                each = []
                for _ in range(args.steps):
                    if arm == "host":
                        dl, fm, nbytes, _ = host_step()
                        each.append(dl + fm)
                        parts[arm].append((dl, fm))
                    else:
                        wall, split, nbytes, up, _ = device_step()
                        each.append(wall)
                        parts[arm].append(split)
                    to_host[arm] = nbytes
                m = sum(each) / len(each)
                means[arm].append(m)
                print(f"{gname:8s} round {r} arm {arm:6s} ms_per_step {m:8.3f}  steps: " + " ".join(f"{x:.2f}" for x in each), flush=True)
        spread = max(means["host"]) - min(means["host"])
        hm, dm = float(np.mean(means["host"])), float(np.mean(means["device"]))
        hp, dp = np.mean(np.array(parts["host"]), axis=0), np.mean(np.array(parts["device"]), axis=0)
        print(f"{gname} host  : {hm * per_10m:8.3f} ms per 10 M reads ({hm:.3f} ms per step, rounds {min(means['host']):.3f}..{max(means['host']):.3f}, spread {spread:.3f} ms): "
              f"download {hp[0]:.3f} ms + format on one thread {hp[1]:.3f} ms; to the host per step: {to_host['host']} bytes of records", flush=True)
        print(f"{gname} device: {dm * per_10m:8.3f} ms per 10 M reads ({dm:.3f} ms per step, rounds {min(means['device']):.3f}..{max(means['device']):.3f}): "
              f"ID upload {dp[0]:.3f} ms + kernels {dp[1]:.3f} ms + copy of the text {dp[2]:.3f} ms; to the host per step: {to_host['device']} bytes of text; "
              f"to the device per step: {up} bytes of IDs and offsets", flush=True)
        print(f"{gname}: device minus host = {(dm - hm) * per_10m:+.3f} ms per 10 M reads; the host arm's spread between rounds is {spread * per_10m:.3f} ms per 10 M reads"
              f" ({'beyond' if abs(dm - hm) > spread else 'within'} the spread)", flush=True)
        b.close()


if __name__ == "__main__":
    main()
