#!/usr/bin/env python3
"""What the lanes of a workspace do to each other, from a rocprofv3 kernel trace of a run with several lanes (the LAST
step: the launches after the last pause of >= 50 ms, as tools/timeline.py cuts it).

For every kernel: launches, summed and mean duration of the launches that ran beside the fused k_edit_myers of another
stream (more than half of their own duration overlaps one) and of those that did not.  And the wall time with one, and
with two or more, fused k_edit_myers launches in flight.

    python3 tools/lane_overlap.py <dir with *_kernel_trace.csv>
"""
import collections
import csv
import glob
import os
import re
import sys


def norm(name):
    name = name.replace("void ", "").replace("mtsv::(anonymous namespace)::", "")
    return re.sub(r"\(.*", "", name)


FUSED = re.compile(r"k_edit_myers<\d+, 3[,>]")


def main():
    d = sys.argv[1]
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), norm(r["Kernel_Name"]), r.get("Stream_Id") or r.get("Queue_Id"))
            for r in csv.DictReader(open(f))]
    rows.sort()
    cut = 0
    for i in range(1, len(rows)):
        if rows[i][0] - max(r[1] for r in rows[max(0, i - 64):i]) > 50e6:
            cut = i
    rows = rows[cut:]
    t0, t1 = rows[0][0], max(r[1] for r in rows)
    fused = [r for r in rows if FUSED.match(r[2])]
    print(f"last step: {len(rows)} launches on {len({r[3] for r in rows})} streams, span {(t1 - t0) / 1e6:.2f} ms, {len(fused)} fused k_edit_myers launches")
    ev = sorted([(s, 1) for s, _, _, _ in fused] + [(e, -1) for _, e, _, _ in fused])
    depth, last, hist = 0, t0, collections.Counter()
    for t, dlt in ev:
        hist[min(depth, 3)] += t - last
        last = t
        depth += dlt
    hist[0] += t1 - last
    print("wall time by fused k_edit_myers launches in flight (0, 1, 2, 3+): " + " ".join(f"{hist[k] / 1e6:.2f}" for k in range(4)) + " ms")
    beside = collections.defaultdict(list)
    alone = collections.defaultdict(list)
    for s, e, k, sid in rows:
        ov = sum(max(0, min(e, fe) - max(s, fs)) for fs, fe, _, fsid in fused if fsid != sid)
        (beside if 2 * ov > e - s else alone)[k].append((e - s) / 1e6)
    print(f"{'kernel':36s} {'beside another lane fused pass':>32s} {'not beside one':>32s}")
    print(f"{'':36s} {'launches':>10s} {'sum ms':>10s} {'mean ms':>10s} {'launches':>10s} {'sum ms':>10s} {'mean ms':>10s}")
    names = sorted(set(beside) | set(alone), key=lambda k: -(sum(beside[k]) + sum(alone[k])))
    for k in names:
        b, a = beside[k], alone[k]
        print(f"{k[:36]:36s} {len(b):10d} {sum(b):10.3f} {(sum(b) / len(b) if b else 0):10.3f} {len(a):10d} {sum(a):10.3f} {(sum(a) / len(a) if a else 0):10.3f}")
    print(f"{'sum':36s} {'':10s} {sum(map(sum, beside.values())):10.3f} {'':10s} {'':10s} {sum(map(sum, alone.values())):10.3f}")


if __name__ == "__main__":
    main()
