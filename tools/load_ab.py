#!/usr/bin/env python3
"""load_ab.py -- what making a chunk resident costs and where: the host pack of mtsv_index_to_device against the pack on the
device (MTSV_DEV_PACK_ON_DEVICE, k_pack.hip), and mtsv-binner --fold-on-gpu with and without --fold-prefetch.

    timeout -k 10 1100 python tools/load_ab.py [--chunks 8] [--upload-chunks 2] [--rounds 3] [--cli-reads 1000000] [--cli-runs 2]

The chunk files are fold_ab.py's (bench.py --mode chunks, BASELINE config 5; built and written when they are not there).

Part (a), in this process, per chunk of the first --upload-chunks: the file is loaded once; then, --rounds times after a warm-up
round, mtsv_index_to_device with MTSV_DEV_DEFAULT and with MTSV_DEV_PACK_ON_DEVICE take turns on that one host index (the flags
differ, so every call frees what is resident and uploads again).  Per call: wall time, and the upload's own split from
mtsv_index_download_device's header -- pack_ms (the host pack by the host's clock, or the pack kernels by device events),
copy_ms (the synchronous copies by the host's clock), accel_build_ms (full suffix array and k-mer table, device events).
Beside them the floors: hipMemcpy of the raw bytes the device pack sends (2 n + 48 n / k) from ordinary memory and from
page-locked memory, what hipHostRegister of n bytes costs, and every pack kernel's device time (a child process under
MTSV_TRACE, whose upload prints them).

Part (b), the command line on --cli-reads reads in a FASTQ file, --cli-runs times each after one warm-up run, alternating:
--fold-on-gpu (arm 1, the parent's path), with MTSV_DEV_PACK=device (arm 2), with --fold-prefetch (arm 3), with both (arm 4).
Wall time of the process and its MTSV_CLI_TIMING line; every arm's four files compared with arm 1's byte for byte."""
import argparse
import ctypes
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
from fold_ab import BINNER, chunk_path, spread  # noqa: E402
from merge_ab import CHUNK_SPEC, load_chunks  # noqa: E402

ARMS = (("host pack", M.DEV_DEFAULT), ("device pack", M.DEV_PACK_ON_DEVICE))


def hip_lib():
    try:
        return ctypes.CDLL("libamdhip64.so")
    except OSError:
        return ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))


def h2d_ms(host_ptr, n_bytes, repeats=3):
    """wall time of a synchronous hipMemcpy host-to-device of n_bytes, per repeat after one warm-up"""
    hip = hip_lib()
    d = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(n_bytes)) != 0:
        raise SystemExit("load_ab: hipMalloc failed")
    out = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        if hip.hipMemcpy(d, ctypes.c_void_p(host_ptr), ctypes.c_size_t(n_bytes), 1) != 0:  # hipMemcpyHostToDevice
            raise SystemExit("load_ab: hipMemcpy failed")
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(d)
    return out


def trace_child(path):
    """one device-pack upload of `path` under MTSV_TRACE: the library prints every pack kernel's device time"""
    ix = M.MGIndex.load(path)
    ix.to_device(0, M.DEV_DEFAULT)          # (warm-up: code objects)
    ix.to_device(0, M.DEV_PACK_ON_DEVICE)
    ix.close()


def part_a(args):
    n = None
    for c in range(args.upload_chunks):
        path = chunk_path(c, args.chunks)
        t0 = time.perf_counter()
        ix = M.MGIndex.load(path)
        load_ms = (time.perf_counter() - t0) * 1e3
        info = ix.info()
        n, k = info["n"], info["occ_k"]
        rec = {name: dict(wall=[], pack_ms=[], copy_ms=[], accel_build_ms=[]) for name, _ in ARMS}
        shape = {}
        for r in range(args.rounds + 1):  # (round 0 warms up)
            for name, flags in ARMS:
                t0 = time.perf_counter()
                ix.to_device(0, flags)
                wall = (time.perf_counter() - t0) * 1e3
                h = ix.download_device(0, M.DEVPART_HEADER)
                assert h["packed_on_device"] == (1 if flags else 0)
                shape[name] = {key: v for key, v in h.items() if key not in ("pack_ms", "copy_ms", "accel_build_ms", "packed_on_device")}
                if r:
                    rec[name]["wall"].append(wall)
                    for key in ("pack_ms", "copy_ms", "accel_build_ms"):
                        rec[name][key].append(h[key])
        ix.close()
        same = shape["host pack"] == shape["device pack"]
        print(f"chunk {c}: n = {n}, Occ interval {k}; mtsv_index_load {load_ms:.1f} ms; headers of the two arms equal (kmer_k {shape['host pack']['kmer_k']}, "
              f"device_bytes {shape['host pack']['device_bytes']}): {same}", flush=True)
        for name, _ in ARMS:
            v = rec[name]
            rest = [w - p - cp - a for w, p, cp, a in zip(v["wall"], v["pack_ms"], v["copy_ms"], v["accel_build_ms"])]
            print(f"  {name}: mtsv_index_to_device {spread(v['wall'])} ms = pack {spread(v['pack_ms'])} + copies {spread(v['copy_ms'])} + "
                  f"accel_build {spread(v['accel_build_ms'])} + the rest (allocations, frees, samples, bins) {spread(rest)}", flush=True)
        if not same:
            sys.exit("load_ab: the two arms left different headers")
    # the floors, on the last chunk's size
    raw = 2 * n + 48 * ((n - 1) // k + 1)
    pageable = np.ones(n, dtype=np.uint8)
    print(f"hipMemcpy of n = {n} bytes from ordinary memory: {spread(h2d_ms(pageable.ctypes.data, n))} ms a copy; the device pack sends {raw} bytes raw, "
          f"the host pack {n // 2 + n} packed (+ the samples and bins in both)", flush=True)
    pinned = M.HostBuffer(n)
    pinned.array[:] = 1
    print(f"hipMemcpy of the same bytes from page-locked memory: {spread(h2d_ms(pinned.array.ctypes.data, n))} ms a copy", flush=True)
    pinned.close()
    reg = []
    for _ in range(3):
        t0 = time.perf_counter()
        M.host_register(pageable)
        t1 = time.perf_counter()
        M.host_unregister(pageable)
        reg.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    print(f"hipHostRegister of n bytes: {spread([a for a, _ in reg])} ms, unregister {spread([b for _, b in reg])} ms", flush=True)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", chunk_path(0, args.chunks)], capture_output=True, text=True,
                       env={**os.environ, "MTSV_TRACE": "1"})
    lines = [ln for ln in p.stderr.splitlines() if "pack on device" in ln]
    print("pack kernels, device time (one upload in a child process): " + (lines[-1] if lines else f"no trace line (exit {p.returncode})"), flush=True)


CLI_ARMS = (("1 fold", [], {}), ("2 fold, MTSV_DEV_PACK=device", [], {"MTSV_DEV_PACK": "device"}), ("3 fold + prefetch", ["--fold-prefetch"], {}),
            ("4 fold + prefetch, MTSV_DEV_PACK=device", ["--fold-prefetch"], {"MTSV_DEV_PACK": "device"}))
TIMING = re.compile(r"index_load ([\d.]+) s, index_to_device ([\d.]+) s, upload_and_run ([\d.]+) s, fold ([\d.]+) s \(device [\d.]+ ms\), results_report_flags ([\d.]+) s"
                    r"(?:; prefetch: loader ([\d.]+) s, waited_for_loader ([\d.]+) s)?")


def part_b(args, fq, d):
    index = ",".join(chunk_path(c, args.chunks) for c in range(args.chunks))
    wall = {name: [] for name, _, _ in CLI_ARMS}
    split = {name: [] for name, _, _ in CLI_ARMS}
    same = True
    for k in range(args.cli_runs + 1):  # (run 0 warms the page cache)
        for a, (name, switches, env) in enumerate(CLI_ARMS):
            out = [os.path.join(d, f"arm{a}.{x}") for x in ("res", "rep", "m", "u")]
            t0 = time.perf_counter()
            p = subprocess.run([BINNER, "--fastq", fq, "-i", index, "-m", out[0], "--force-overwrite", "--fold-on-gpu", *switches, "--report", out[1],
                                "--matched", out[2], "--unmatched", out[3]], capture_output=True, text=True, env={**os.environ, "MTSV_CLI_TIMING": "1", **env})
            dt = (time.perf_counter() - t0) * 1e3
            if p.returncode != 0:
                sys.exit(f"load_ab: mtsv-binner arm {name} failed:\n{p.stdout}{p.stderr}")
            m = TIMING.search(p.stderr)
            if k and m:
                wall[name].append(dt)
                split[name].append([float(x) if x else 0.0 for x in m.groups()])
            if a:
                same = same and all(subprocess.run(["cmp", "-s", o, o.replace(f"arm{a}.", "arm0.")]).returncode == 0 for o in out)
    print(f"command line on {args.cli_reads} reads, {args.chunks} chunks, {args.cli_runs} runs an arm after a warm-up run, alternating; every arm's files equal arm 1's (cmp): {same}", flush=True)
    for name, _, _ in CLI_ARMS:
        sp = np.array(split[name])
        cols = ("index_load (under prefetch: the wait)", "index_to_device", "upload_and_run", "fold", "results_report_flags", "loader", "waited_for_loader")
        print(f"  arm {name}: {spread(wall[name])} ms per process; " + ", ".join(f"{cname} {spread(list(sp[:, i]))} s" for i, cname in enumerate(cols)), flush=True)
    if not same:
        sys.exit("load_ab: an arm's files differ from arm 1's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--upload-chunks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cli-reads", type=int, default=1_000_000)
    ap.add_argument("--cli-runs", type=int, default=2)
    ap.add_argument("--trace-child", default="")
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("load_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    if args.trace_child:
        return trace_child(args.trace_child)
    K, read_len = args.chunks, CHUNK_SPEC[4]
    t0 = time.perf_counter()
    chunks = load_chunks(K)  # (builds and writes the files when they are missing; all resident for the reads' sampling)
    print(f"{K} chunk files ready after {time.perf_counter() - t0:.1f} s", flush=True)
    d = f"/tmp/mtsv_load_ab_{os.getpid()}"
    os.makedirs(d, exist_ok=True)
    fq = os.path.join(d, "reads.fastq")
    if args.cli_runs > 0 and args.cli_reads > 0:
        qual = b"I" * read_len
        with open(fq, "wb") as fh:
            i = 0
            for c in range(K):
                share = args.cli_reads // K + (1 if c < args.cli_reads % K else 0)
                part, _ = M.synth_reads(chunks[c], seed=2000 + c, n_reads=share, read_len=read_len)
                for row in np.asarray(part).reshape(share, read_len):
                    fh.write(b"@r%d\n" % i + row.tobytes() + b"\n+\n" + qual + b"\n")
                    i += 1
    for ix in chunks:
        ix.close()
    part_a(args)
    if args.cli_runs > 0 and args.cli_reads > 0:
        part_b(args, fq, d)
    for name in os.listdir(d):
        os.remove(os.path.join(d, name))
    os.rmdir(d)


if __name__ == "__main__":
    main()
