#!/usr/bin/env python3
"""Static instruction counts of one kernel, per basic block, from the compiler's assembly -- no GPU needed.

    cd mtsv_tools_amd/csrc
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize --cuda-device-only -S k_verify.hip -o k_verify.s
    python3 ../../tools/asm_blocks.py k_verify.s 'k_edit_myers<5, 3>'
    python3 ../../tools/asm_blocks.py k_verify.s 'k_edit_myers<5, 3>' --sum .LBB46_9 .LBB46_23

(the Makefile's HIPFLAGS plus `--cuda-device-only -S`).  The kernel is named by a substring of its demangled name.  Every
block is printed in program order with its VALU (v_*), SALU (s_* but waits, nops and branches), vector memory
(global_/flat_/buffer_/scratch_), scalar memory (s_load_/s_buffer_load_), LDS (ds_*) and branch counts, and the labels its
branches go to, so that loops (a branch to an earlier block) can be told from straight-line code.  --sum FIRST LAST adds up
the blocks from FIRST to LAST in program order, both included.  In k_edit_myers the set-up of an item's match masks runs
from the block that takes the item (the first one with vector loads: work list, candidate, offsets) to the last block that
stores to LDS (column lds_st: eq_tab is written nowhere else); the column loop's blocks follow it, 65 VALU each for W = 5."""
import argparse
import re
import subprocess
import sys

CLASSES = ("valu", "salu", "vmem", "smem", "lds", "branch", "other")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return out.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def classify(op):
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep", "s_setprio", "s_inst_prefetch", "s_code_end")):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def kernel_bodies(path):
    """{mangled name: [lines]} of every function of the file"""
    bodies, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                bodies[cur].append(line)
    return bodies


def blocks_of(lines):
    """[(label, counts, lds_writes, targets)] in program order"""
    blocks = [["entry", dict.fromkeys(CLASSES, 0), 0, []]]
    for line in lines:
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                blocks.append([m.group(1), dict.fromkeys(CLASSES, 0), 0, []])
            continue
        op = s.split()[0]
        c = classify(op)
        blocks[-1][1][c] += 1
        if op.startswith(("ds_write", "ds_st")):
            blocks[-1][2] += 1
        if c == "branch":
            blocks[-1][3] += re.findall(r"\.LBB\d+_\d+", s)
    return blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the demangled kernel name")
    ap.add_argument("--sum", nargs=2, metavar=("FIRST", "LAST"))
    ap.add_argument("--min", type=int, default=0, help="print only blocks with at least this many instructions")
    args = ap.parse_args()
    bodies = kernel_bodies(args.asm)
    names = list(bodies)
    hits = [(m, d) for m, d in zip(names, demangle(names)) if args.kernel in d]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {args.kernel!r}: " + "; ".join(d for _, d in hits[:8]))
    mangled, shown = hits[0]
    blocks = blocks_of(bodies[mangled])
    print(f"# {shown}: {len(blocks)} blocks")
    print(f"# {'block':<12}" + "".join(f"{c:>8}" for c in CLASSES) + "  lds_st  branches to")
    order = {b[0]: i for i, b in enumerate(blocks)}
    for i, (label, cnt, st, tg) in enumerate(blocks):
        if sum(cnt.values()) < args.min:
            continue
        back = ["^" + t if order.get(t, i + 1) <= i else t for t in tg]
        print(f"{label:<14}" + "".join(f"{cnt[c]:>8}" for c in CLASSES) + f"{st:>8}  " + " ".join(back))
    tot = {c: sum(b[1][c] for b in blocks) for c in CLASSES}
    print(f"{'total':<14}" + "".join(f"{tot[c]:>8}" for c in CLASSES))
    span = None
    if args.sum:
        span = (order[args.sum[0]], order[args.sum[1]])
    if span:
        part = {c: sum(b[1][c] for b in blocks[span[0]:span[1] + 1]) for c in CLASSES}
        print(f"{blocks[span[0]][0]}..{blocks[span[1]][0]} ({span[1] - span[0] + 1} blocks)".ljust(14)
              + "".join(f"{part[c]:>8}" for c in CLASSES))


if __name__ == "__main__":
    main()
