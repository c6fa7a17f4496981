#!/usr/bin/env python3
"""merge_ab.py -- what merging the chunks' hits per read on the device (k_merge.hip, mtsv_batch_copy_reads,
mtsv_batch_merge_runs) costs and saves, beside the host merge of mtsv_bin_batch_chunks, inside one process.

    timeout -k 10 900 python tools/merge_ab.py [--chunks 8] [--reads N] [--block-reads 1048576] [--steps 5] [--warmup 2] [--rounds 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/merge_ab.py --trace-run device

The workload is that of `bench.py --mode chunks` on one GPU: --chunks synthetic database chunks (bench.py's index files,
built and written when they are not there), all resident on device 0, and a step's reads sampled from every chunk in equal
shares.  Two ways through a step, in turn, --rounds times --steps steps each:

  host    one call of mtsv_bin_batch_chunks on the step's reads: every chunk receives the reads over PCIe, every chunk's hits
          go to the host, the host merges them per read (the path before the device merge existed: the yardstick)
  device  the step's reads in blocks of --block-reads: mtsv_batch_upload to the first chunk's workspace,
          mtsv_batch_copy_reads to the others, mtsv_batch_run on each, mtsv_batch_merge_runs into a collector,
          mtsv_batch_download -- what mtsv-binner --merge-on-gpu does per block of reads

Both end with the same hits (checked once).  Printed: every round's mean and every step; per way the time per step with the
rounds' spread; the device time of the merge kernels (device_ms of mtsv_batch_merge_runs, summed over a step's blocks)
beside a hipMemcpyDtoD of the merged bytes, timed with HIP events in the same process; the bytes over PCIe per step in each
direction.

--trace-run ARM: one warm-up and three steps of that arm alone, for a kernel trace."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mtsv_tools_amd as M  # noqa: E402
from mtsv_tools_amd import _lib as L  # noqa: E402
from chain_ab import dtod_ms  # noqa: E402

SEED_DB = 0x6D747376                                   # bench.py's
CHUNK_SPEC = (128, 4, 674_000, 10_000_000, 150)        # bench.py's: per chunk taxa, GIs per taxon, sequence length; reads, read length


def load_chunks(n_chunks):
    """bench.py --mode chunks' index files: chunk c is its own synthetic database (a seed per chunk)"""
    n_taxa, gis, seq_len, _, _ = CHUNK_SPEC
    out = []
    for c in range(n_chunks):
        path = f"/tmp/mtsv_bench_config5_c{c}of{n_chunks}.idx"
        ok = False
        try:
            ok = os.path.exists(path) and int.from_bytes(open(path, "rb").read(8), "little") == n_taxa * gis * seq_len + 1
        except OSError:
            pass
        if not ok:
            M.set_build_device(0)
            ixb = M.MGIndex.synth(SEED_DB + 101 * (c + 1), n_taxa, gis, seq_len, threads=min(32, os.cpu_count() or 8))
            M.set_build_device(-1)
            ixb.write(path + ".tmp")
            ixb.close()
            os.replace(path + ".tmp", path)
        ix = M.MGIndex.load(path)
        ix.to_device(0)
        out.append(ix)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--block-reads", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-run", choices=["host", "device"], default=None)
    args = ap.parse_args()
    if M.device_count() < 1:
        sys.exit("merge_ab.py needs a HIP device: libmtsv_amd has no CPU path")
    n_reads, read_len = args.reads or CHUNK_SPEC[3], CHUNK_SPEC[4]
    K = args.chunks
    chunks = load_chunks(K)
    share = [n_reads // K + (1 if c < n_reads % K else 0) for c in range(K)]
    pinned = M.HostBuffer(n_reads * read_len)
    at = 0
    for c in range(K):
        part, _ = M.synth_reads(chunks[c], seed=2000 + c, n_reads=share[c], read_len=read_len)
        pinned.array[at:at + len(part)] = part
        at += len(part)
    bases = pinned.array
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    params = M.default_params()
    print(f"{K} chunks of n = {chunks[0].info()['n']:.3g} symbols on device 0; {n_reads} reads of {read_len} bases per step; "
          f"device arm in blocks of {args.block_reads} reads", flush=True)
    handles = (ctypes.c_void_p * K)(*[ix.h for ix in chunks])
    devs = (ctypes.c_int * K)(*([0] * K))

    def host_step():
        t0 = time.perf_counter()
        out_p, out_n = ctypes.c_void_p(), ctypes.c_uint64()
        L._check(M.lib().mtsv_bin_batch_chunks(handles, devs, K, bases.ctypes.data, off.ctypes.data, n_reads, ctypes.byref(params),
                                               ctypes.byref(out_p), ctypes.byref(out_n)))
        t1 = time.perf_counter()
        hits = L._hits_from(out_p, out_n.value)
        return hits, dict(step=(t1 - t0) * 1e3, merge_ms=0.0, n_hits=len(hits), h2d=K * (n_reads * read_len + 4 * (n_reads + 1)), d2h=32 * len(hits))

    B = min(args.block_reads, n_reads)
    ws, dst = None, None

    def device_setup():
        nonlocal ws, dst
        if ws is None:
            ws = [M.Batch(ix, 0, B, B * read_len, lanes=1) for ix in chunks]
            dst = M.Batch(chunks[0], 0, 1024, 1 << 16, lanes=1)

    def device_step():
        device_setup()
        t0 = time.perf_counter()
        parts, merge_ms, h2d, d2h = [], 0.0, 0, 0
        for a in range(0, n_reads, B):
            b = min(n_reads, a + B)
            ws[0].upload(bases[a * read_len:b * read_len], off[a:b + 1] - off[a])
            for w in ws[1:]:
                w.copy_reads(ws[0])
            for w in ws:
                w.run(params)
            merge_ms += dst.merge_runs(ws)
            h = dst.download()
            h["read"] += np.uint64(a)
            parts.append(h)
            h2d += (b - a) * read_len + 4 * (b - a + 1) + 32 * K
            d2h += 32 * len(h) + 16
        t1 = time.perf_counter()
        hits = np.concatenate(parts) if len(parts) > 1 else parts[0]
        return hits, dict(step=(t1 - t0) * 1e3, merge_ms=merge_ms, n_hits=len(hits), h2d=h2d, d2h=d2h)

    ways = (("host", host_step), ("device", device_step))
    if args.trace_run:
        step = dict(ways)[args.trace_run]
        for _ in range(4):
            hits, f = step()
        print(f"trace run: one warm-up and three {args.trace_run} steps, {len(hits)} hits per step", flush=True)
        return

    hits_a, fa = host_step()
    hits_b, fb = device_step()
    same = len(hits_a) == len(hits_b) and all(np.array_equal(hits_a[f], hits_b[f]) for f in M.HIT_DTYPE.names)
    print(f"{len(hits_a)} merged hits per step; hits of the two ways identical: {same}", flush=True)
    if not same:
        sys.exit("merge_ab: the host merge and the device merge disagree")
    del hits_a, hits_b

    means = {name: [] for name, _ in ways}
    parts = {name: [] for name, _ in ways}
    for r in range(1, args.rounds + 1):
        for name, step in ways:
            for _ in range(args.warmup if r == 1 else 1):
                step()
            each = [step()[1] for _ in range(args.steps)]
            parts[name] += each
            m = sum(f["step"] for f in each) / len(each)
            means[name].append(m)
            print(f"round {r} {name:6s} ms_per_step {m:9.3f}  steps: " + " ".join(f"{f['step']:.2f}" for f in each), flush=True)
    for name, _ in ways:
        p = parts[name]
        print(f"{name:6s}: {np.mean(means[name]):9.3f} ms per step (rounds {min(means[name]):.3f}..{max(means[name]):.3f}); per step "
              f"{p[-1]['h2d']} bytes to the device, {p[-1]['d2h']} to the host", flush=True)
    dev = [f["merge_ms"] for f in parts["device"]]
    nb = 32 * fb["n_hits"]
    copy_ms = dtod_ms(nb)
    print(f"merge kernels: {np.mean(dev):.3f} ms of device time per step (min {min(dev):.3f}, max {max(dev):.3f}) for {nb} merged bytes in "
          f"{(n_reads + B - 1) // B} merges of {K} sources; hipMemcpyDtoD of {nb} bytes: {copy_ms:.3f} ms ({nb / copy_ms / 1e6:.0f} GB/s); the kernels take "
          f"{np.mean(dev) / copy_ms:.2f} times the plain copy", flush=True)
    d, h = np.mean(means["device"]), np.mean(means["host"])
    spread = max(means["host"]) - min(means["host"])
    verdict = "cannot be told apart from" if abs(d - h) < 2 * spread else ("is faster than" if d < h else "is SLOWER than")
    print(f"end to end the device arm {verdict} the host arm: {d:.3f} against {h:.3f} ms per step (the host arm's rounds spread {spread:.3f} ms)", flush=True)
    for b in (ws or []) + ([dst] if dst else []):
        b.close()
    pinned.close()


if __name__ == "__main__":
    main()
