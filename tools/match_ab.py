#!/usr/bin/env python3
"""match_ab.py -- what the match flags (k_match.hip) cost or save a step, measured through the library as bench.py does.

    python tools/match_ab.py [--workload config2] [--steps 20] [--warmup 5] [--rounds 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/match_ab.py --trace-run off|with_hits|only

The same index file, reads and workspace as bench.py's timed region (host path: mtsv_batch_run_host + mtsv_batch_download on
reads in page-locked memory).  The three modes -- MTSV_MATCH_OFF, MTSV_MATCH_WITH_HITS, MTSV_MATCH_ONLY -- alternate, --rounds
times --steps steps each, in one process on one box; a step with the flags on ends with mtsv_batch_match_flags, as a caller's
would.  Every round's mean and every step are printed, then per mode: the time per 10 M reads, its difference to the off
rounds beside their spread (a difference below twice that spread cannot be told apart), the device time of k_match per step
(HIP events around its launches, summed like the taxa report's) and the bytes a step copies back to the host (32 per hit,
8 per 64 reads of flags and 8 for the counter).

--trace-run: one warm-up and three steps in one mode, for a kernel trace (a default run must show no k_match launch; a
flags-only run neither k_gather nor the scan before it)."""
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

MODES = (("off", M.MATCH_OFF), ("with_hits", M.MATCH_WITH_HITS), ("only", M.MATCH_ONLY))


def set_mode(b, mode):
    """the library decides when the flags are switched on whether it will say what k_match took"""
    os.environ["MTSV_TRACE"] = "1"
    try:
        b.set_match_flags(mode)
    finally:
        del os.environ["MTSV_TRACE"]


def kernel_ms(b):
    """mtsv_batch_match_flags with the library's "[match] ..." line caught: (flags, n_matched, launches, device ms, bytes)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            flags, n_matched = b.match_flags()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"\[match\] (\d+) kernel launches, ([0-9.]+) ms, .* (\d+) bytes of flags", text)
    if not m:
        raise SystemExit("match_ab: the library printed no [match] line: " + text)
    return flags, n_matched, int(m.group(1)), float(m.group(2)), int(m.group(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--trace-run", choices=[m for m, _ in MODES], default=None)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("match_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    ix, n_reads, read_len, desc = load_index(args.workload)
    if args.reads:
        n_reads = args.reads
    bases, off = M.synth_reads(ix, seed=1000, n_reads=n_reads, read_len=read_len)
    print(f"{args.workload}: {desc}; {n_reads} reads per step", flush=True)
    params = M.default_params()
    slice_reads = M.bin_batch_slice_reads(n_reads)
    hb = M.Batch(ix, 0, min(n_reads, slice_reads), min(len(bases), slice_reads * (read_len + 8)))
    pinned = M.HostBuffer(len(bases))
    pinned.array[:] = bases
    bases_p, off_p = pinned.array.ctypes.data, off.ctypes.data
    words_p, n_p, m_p = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()

    def step(mode):
        L._check(M.lib().mtsv_batch_run_host(hb.h, bases_p, off_p, n_reads, ctypes.byref(params)))
        out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
        L._check(M.lib().mtsv_batch_download(hb.h, ctypes.byref(out_p), ctypes.byref(out_n)))
        M.lib().mtsv_hits_free(out_p)
        if mode != M.MATCH_OFF:
            L._check(M.lib().mtsv_batch_match_flags(hb.h, ctypes.byref(words_p), ctypes.byref(n_p), ctypes.byref(m_p)))
            M.lib().mtsv_free(words_p)
        return out_n.value

    if args.trace_run:
        mode = dict(MODES)[args.trace_run]
        hb.set_match_flags(mode)
        for _ in range(4):
            n_hits = step(mode)
        print(f"trace run, mode {args.trace_run}: one warm-up and three steps, {n_hits} hits per step", flush=True)
        return

    per_10m = 1e7 / n_reads
    means = {name: [] for name, _ in MODES}
    facts = {}
    for r in range(1, args.rounds + 1):
        for name, mode in MODES:
            hb.set_match_flags(M.MATCH_OFF)
            if mode != M.MATCH_OFF:
                set_mode(hb, mode)
            for _ in range(args.warmup if r == 1 else 2):
                step(mode)
            each = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                n_hits = step(mode)
                each.append((time.perf_counter() - t0) * 1e3)
            m = sum(each) / len(each)
            means[name].append(m)
            print(f"round {r} flags {name:9s} ms_per_step {m:7.3f}  steps: " + " ".join(f"{x:.2f}" for x in each), flush=True)
            if mode != M.MATCH_OFF:
                flags, n_matched, launches, ms, flag_bytes = kernel_ms(hb)   # (of the last step)
                assert len(flags) == n_reads and int(flags.sum()) == n_matched
                facts[name] = (n_hits, n_matched, launches, ms, flag_bytes)
            else:
                facts[name] = (n_hits, None, 0, 0.0, 0)
    off_m = float(np.mean(means["off"]))
    spread = max(means["off"]) - min(means["off"])
    print(f"off rounds {min(means['off']):.3f}..{max(means['off']):.3f} ms per step, spread {spread:.3f} ms; twice the spread = {2 * spread:.3f} ms")
    for name, _ in MODES:
        mm = float(np.mean(means[name]))
        n_hits, n_matched, launches, ms, flag_bytes = facts[name]
        print(f"flags {name:9s}: {mm * per_10m:8.3f} ms per 10 M reads ({mm:.3f} ms per step, rounds {min(means[name]):.3f}..{max(means[name]):.3f}); "
              f"minus off = {(mm - off_m) * per_10m:+.3f} ms per 10 M reads; k_match {launches} launches, {ms:.3f} ms of device time per step; "
              f"to the host per step: {32 * n_hits} bytes of hits + {flag_bytes} bytes of flags"
              + (f"; {n_matched} of {n_reads} reads matched" if n_matched is not None else ""), flush=True)
    hb.close()
    pinned.close()


if __name__ == "__main__":
    main()
