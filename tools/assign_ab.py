#!/usr/bin/env python3
"""assign_ab.py -- what the assignments (k_collapse.hip) cost or save a step, measured through the library as bench.py does.

    python tools/assign_ab.py [--workload config2] [--steps 10] [--warmup 3] [--rounds 3] [--grain taxid|taxid-gi|long] [--format]

The same index file and reads as bench.py.  The three modes -- MTSV_ASSIGN_OFF, MTSV_ASSIGN_WITH_HITS, MTSV_ASSIGN_ONLY --
alternate, --rounds times --steps steps each, in one process on one box, on both paths: the host path (bench.py's timed
region: mtsv_batch_run_host on reads in page-locked memory, then the downloads a caller of that mode makes) and the resident
path (mtsv_batch_upload once, then mtsv_batch_run and the downloads).  A step with the assignments on ends with
mtsv_batch_download_assignments; in MTSV_ASSIGN_ONLY mtsv_batch_download is still called and returns nothing.

Every round's mean and every step are printed, then per path and mode: the time per 10 M reads, its difference to the off
rounds beside their spread (a difference below twice that spread cannot be told apart), the device time of the collapse
kernels per step (HIP events around them, summed over passes and lanes: the mean and the range over all timed steps, and
every step's figure on its round's line), the stage times of the same step that serve as
comparison points -- stage 6, scan + k_gather, and k_report's device time from a step with the taxa report on -- the reads every tier took (the library's "[collapse]" line) and the bytes a
step copies back to the host (32 per hit, 16 or 24 per assignment).  Last, a hipMemcpyDtoD of one step's hit bytes, the floor
for any kernel that reads the hits once.

--grain puts the workspaces in that grain of the assignments (mtsv_batch_set_assignment_grain) before anything is switched
on: taxid is the default and what the tool always did; taxid-gi and long are the 24-byte records, downloaded with
mtsv_batch_download_assignments_gi.  --format makes every step end with the result text a caller would write: from the
hits (mtsv_format_results, long lines under a wide grain) where the step downloaded hits, from the records
(mtsv_format_assignments, _gi) in MTSV_ASSIGN_ONLY -- hits plus host formatting against records plus their formatting."""
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

MODES = (("off", M.ASSIGN_OFF), ("with_hits", M.ASSIGN_WITH_HITS), ("only", M.ASSIGN_ONLY))
GRAINS = {"taxid": M.GRAIN_TAXID, "taxid-gi": M.GRAIN_TAXID_GI, "long": M.GRAIN_LONG}
LINE = re.compile(r"\[collapse\] run: (\d+) launches, ([0-9.]+) ms, (\d+) hits -> (\d+) assignments; reads by tier: lane (\d+), wavefront (\d+), lds (\d+), global (\d+)")


def traced(fn, set_env=False):
    """fn() with stderr caught (set_env: and MTSV_TRACE set): (its result, the text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    if set_env:
        os.environ["MTSV_TRACE"] = "1"
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("MTSV_TRACE", None)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def dtod_floor_ms(n_bytes, reps=20):
    """a device-to-device copy of n_bytes through torch's allocator (hipMemcpyDtoD), ms per copy"""
    import torch
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        b.copy_(a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--grain", choices=list(GRAINS), default="taxid")
    ap.add_argument("--format", action="store_true")
    args = ap.parse_args()
    grain = GRAINS[args.grain]
    wide = grain != M.GRAIN_TAXID
    rec_bytes = 24 if wide else 16
    if M.device_count() < 1:
        sys.exit("assign_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    ix, n_reads, read_len, desc = load_index(args.workload)
    if args.reads:
        n_reads = args.reads
    bases, off = M.synth_reads(ix, seed=1000, n_reads=n_reads, read_len=read_len)
    print(f"{args.workload}: {desc}; {n_reads} reads per step" + (f"; grain {args.grain}" if wide else "") + ("; steps format their result" if args.format else ""),
          flush=True)
    params = M.default_params()
    slice_reads = M.bin_batch_slice_reads(n_reads)
    pinned = M.HostBuffer(len(bases))
    pinned.array[:] = bases
    bases_p, off_p = pinned.array.ctypes.data, off.ctypes.data
    per_10m = 1e7 / n_reads
    if args.format:
        ids_blob = b"".join(b"r%d\0" % i for i in range(n_reads))
        id_off = np.zeros(n_reads + 1, dtype=np.uint64)
        np.cumsum([len(b"r%d" % i) + 1 for i in range(n_reads)], out=id_off[1:])

    def formatted(fn, records, n, from_hits=False):
        """the result text of a step, made and freed"""
        if not args.format:
            return
        out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
        L._check(fn(records, n, ids_blob, id_off.ctypes.data, n_reads, *([int(wide)] if from_hits else []),
                    ctypes.byref(out_p), ctypes.byref(out_n)))
        M.lib().mtsv_free(out_p)

    def downloads(b, mode):
        out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
        L._check(M.lib().mtsv_batch_download(b.h, ctypes.byref(out_p), ctypes.byref(out_n)))
        if mode != M.ASSIGN_ONLY:
            formatted(M.lib().mtsv_format_results, out_p, out_n.value, True)
        M.lib().mtsv_hits_free(out_p)
        n_assign, ms = 0, 0.0
        if mode != M.ASSIGN_OFF:
            a_p, a_n, a_ms = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_float()
            get = M.lib().mtsv_batch_download_assignments_gi if wide else M.lib().mtsv_batch_download_assignments
            L._check(get(b.h, ctypes.byref(a_p), ctypes.byref(a_n), ctypes.byref(a_ms)))
            if mode == M.ASSIGN_ONLY:
                formatted(M.lib().mtsv_format_assignments_gi if wide else M.lib().mtsv_format_assignments, a_p, a_n.value)
            M.lib().mtsv_free(a_p)
            n_assign, ms = a_n.value, a_ms.value
        return out_n.value, n_assign, ms

    def host_step(b, mode):
        L._check(M.lib().mtsv_batch_run_host(b.h, bases_p, off_p, n_reads, ctypes.byref(params)))
        return downloads(b, mode)

    def resident_step(b, mode):
        L._check(M.lib().mtsv_batch_run(b.h, ctypes.byref(params)))
        return downloads(b, mode)

    n_hits_step = 0
    for path, make, step in (("host", lambda: M.Batch(ix, 0, min(n_reads, slice_reads), min(len(bases), slice_reads * (read_len + 8))), host_step),
                             ("resident", lambda: M.Batch(ix, 0, n_reads, len(bases)), resident_step)):
        b = make()
        b.set_assignment_grain(grain)
        if path == "resident":
            b.upload(bases, off)
        means = {name: [] for name, _ in MODES}
        dev_ms = {name: [] for name, _ in MODES}   # the collapse kernels' device time of every timed step
        facts = {}
        for r in range(1, args.rounds + 1):
            for name, mode in MODES:
                b.set_assignments(M.ASSIGN_OFF)
                if mode != M.ASSIGN_OFF:
                    traced(lambda: b.set_assignments(mode), True)     # (the library decides then whether it will print its line)
                for _ in range(args.warmup if r == 1 else 1):
                    step(b, mode)
                each = []
                for _ in range(args.steps - 1):
                    t0 = time.perf_counter()
                    dev_ms[name].append(step(b, mode)[2])
                    each.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                (n_hits, n_assign, ms), text = traced(lambda: step(b, mode))   # the last step with the library's line caught
                each.append((time.perf_counter() - t0) * 1e3)
                dev_ms[name].append(ms)
                m = sum(each) / len(each)
                means[name].append(m)
                st = b.stats()
                n_hits_step = max(n_hits_step, st["n_hits"])
                tiers = LINE.search(text)
                if mode != M.ASSIGN_OFF and not tiers:
                    raise SystemExit("assign_ab: the library printed no [collapse] line: " + text[-400:])
                to_host = 32 * n_hits + rec_bytes * n_assign
                facts[name] = (st["n_hits"], n_assign, ms, list(st["stage_ms"].values())[6], tiers.groups() if tiers else None, to_host)
                print(f"{path:8s} round {r} assignments {name:9s} ms_per_step {m:7.3f}  steps: " + " ".join(f"{x:.2f}" for x in each)
                      + ("  collapse ms: " + " ".join(f"{x:.3f}" for x in dev_ms[name][-args.steps:]) if mode != M.ASSIGN_OFF else ""), flush=True)
        off_m = float(np.mean(means["off"]))
        spread = max(means["off"]) - min(means["off"])
        print(f"{path}: off rounds {min(means['off']):.3f}..{max(means['off']):.3f} ms per step, spread {spread:.3f} ms; twice the spread = {2 * spread:.3f} ms")
        for name, _ in MODES:
            mm = float(np.mean(means[name]))
            n_hits, n_assign, ms, gather_ms, tiers, to_host = facts[name]
            line = (f"{path} assignments {name:9s}: {mm * per_10m:8.3f} ms per 10 M reads ({mm:.3f} ms per step, rounds {min(means[name]):.3f}..{max(means[name]):.3f}); "
                    f"minus off = {(mm - off_m) * per_10m:+.3f} ms per 10 M reads; collapse kernels {float(np.mean(dev_ms[name])):.3f} ms of device time per step "
                    f"({min(dev_ms[name]):.3f}..{max(dev_ms[name]):.3f} over {len(dev_ms[name])} timed steps) beside "
                    f"{gather_ms:.3f} ms of scan + k_gather; {n_hits} hits, {n_assign} assignments; to the host per step: {to_host} bytes")
            if tiers:
                line += f"; {tiers[0]} launches; reads by tier: lane {tiers[4]}, wavefront {tiers[5]}, lds {tiers[6]}, global {tiers[7]}"
            print(line, flush=True)
        # k_report's device time on the same reads, as a comparison point: one step with the taxa report on
        b.set_assignments(M.ASSIGN_OFF)
        b.set_taxa_report(True)
        step(b, M.ASSIGN_OFF)
        _, _, report_ms = b.taxa_report(reset=True)
        print(f"{path}: k_report {report_ms:.3f} ms of device time per step", flush=True)
        b.close()
    pinned.close()
    try:
        print(f"floor: hipMemcpyDtoD of one step's hits ({32 * n_hits_step} bytes): {dtod_floor_ms(32 * n_hits_step):.3f} ms", flush=True)
    except Exception as e:  # (torch without a device build: the floor is left out, the rest stands)
        print(f"floor: not measured ({e})", flush=True)


if __name__ == "__main__":
    main()
