"""What of the chunk merge needs no GPU: the header's declarations, the Python restatement of the merge against hand-made
cases, and the argument rules of mtsv-binner --merge-on-gpu, which are decided before any index is opened."""
import os
import re
import subprocess

import numpy as np

import chunk_merge_ref as CM
import taxa_report_ref as R
from mtsv_tools_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def hits(rows):
    a = np.zeros(len(rows), dtype=O.HIT_DTYPE)
    for k, (read, tax, gi, edit, strand, offset) in enumerate(rows):
        a[k] = (read, tax, gi, edit, strand, offset)
    return a


def test_header_declares_both_functions():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+mtsv_batch_copy_reads\s*\(\s*mtsv_batch\s*\*\s*dst\s*,\s*mtsv_batch\s*\*\s*src\s*,\s*float\s*\*\s*device_ms\s*\)\s*;", src)
    assert re.search(r"int\s+mtsv_batch_merge_runs\s*\(\s*mtsv_batch\s*\*\s*dst\s*,\s*mtsv_batch\s*\*\s*const\s*\*\s*srcs\s*,\s*int\s+n_srcs\s*,"
                     r"\s*float\s*\*\s*device_ms\s*\)\s*;", src)
    for name in ("mtsv_batch_copy_reads", "mtsv_batch_merge_runs"):
        assert name in _lib.EXPORTS


def test_restatement_on_hand_made_cases():
    # chunk 0: reads 0 and 2; chunk 1: reads 1 and 2; chunk 2: read 2 and read 5 -- read 3 and 4 have no hit anywhere
    a = hits([(0, 7, 1, 3, 0, 10), (0, 9, 2, 1, 1, 11), (2, 7, 1, 5, 0, 12)])
    b = hits([(1, 8, 3, 0, 0, 20), (2, 7, 4, 2, 1, 21), (2, 6, 5, 2, 0, 22)])
    c = hits([(2, 6, 6, 4, 0, 30), (5, 1, 7, 9, 1, 31)])
    m = CM.merge_hits([a, b, c])
    assert m["offset"].tolist() == [10, 11, 20, 12, 21, 22, 30, 31]           # read order, chunk order, the chunk's own order
    assert m["read"].tolist() == [0, 0, 1, 2, 2, 2, 2, 5]
    assert CM.presence(m, 6).tolist() == [True, True, True, False, False, True]
    # TaxID 7 of read 2 is in chunks 0 and 1, and the LATER chunk has the smaller edit: the merged read counts it at 2,
    # which ties it with TaxID 6 -- the per-chunk classifications say something else
    stats, total = R.classify_hits(m)
    assert total == 4
    assert stats[6] == [0, 0, 1, 0]                                           # read 2: 7 and 6 tie at edit 2
    assert stats[7] == [0, 0, 1, 1] and stats[9] == [0, 1, 0, 0]              # read 0: 9 (edit 1) beats 7 (edit 3)
    assert stats[8] == [1, 0, 0, 0] and stats[1] == [1, 0, 0, 0]
    per_chunk_total = sum(R.classify_hits(p)[1] for p in (a, b, c))
    assert per_chunk_total == 6 != total                                       # per-chunk counters do not add up
    sa = R.classify_hits(a)[0]
    assert sa[7] == [1, 0, 0, 1]                                               # chunk 0 alone: 7 is read 2's only hit, read 0's worse one
    several, differ, only, none = CM.chunk_facts([a, b, c], 6)
    assert (several, differ, only, none) == (1, 1, [1, 1, 1], 2)
    # one chunk: the list itself; chunks without hits; no hit at all
    assert CM.merge_hits([a]).tolist() == a.tolist()
    e = hits([])
    assert CM.merge_hits([e, b, e]).tolist() == b.tolist()
    assert len(CM.merge_hits([e, e])) == 0
    # the same (read, TaxID, GI, offset) from two chunks stays twice, first chunk first
    d = hits([(2, 7, 1, 9, 0, 12)])
    assert CM.merge_hits([a, d])["edit"].tolist() == [3, 1, 5, 9]


def binner(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_merge_on_gpu_argument_rules_are_decided_before_any_index_is_opened(tmp_path):
    """every run names index files that do not exist: a run that got as far as loading one would exit 2"""
    res, fq = tmp_path / "res", tmp_path / "x.fastq"
    two = f"{tmp_path}/a.idx,{tmp_path}/b.idx"
    r = binner("--fastq", fq, "-i", tmp_path / "a.idx", "-m", res, "--merge-on-gpu")
    assert r.returncode == 1 and "--merge-on-gpu" in r.stderr and "chunks" in r.stderr
    r = binner("--fastq", fq, "-i", f"{tmp_path}/a.idx,", "-m", res, "--merge-on-gpu")          # one entry and a comma
    assert r.returncode == 1 and "--merge-on-gpu" in r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--merge-on-gpu", "--devices", "0,1")
    assert r.returncode == 1 and "--merge-on-gpu" in r.stderr and "--devices" in r.stderr
    # --filter-index with a chunk list stays refused, with the switch too
    r = binner("--fastq", fq, "-i", two, "-m", res, "--merge-on-gpu", "--filter-index", tmp_path / "f.idx")
    assert r.returncode == 1 and "index chunks" in r.stderr
    assert not res.exists()
    # with the switch and a proper chunk list the report and the partition files are accepted: the run gets as far as its input
    r = binner("--fastq", fq, "-i", two, "-m", res, "--merge-on-gpu", "--report", tmp_path / "rep.tsv", "--matched", tmp_path / "m")
    assert r.returncode == 2, r.stderr
    r = binner("--fastq", fq, "-i", two, "--merge-on-gpu", "--unmatched", tmp_path / "u", "--devices", "0")
    assert r.returncode == 2, r.stderr
    # without it they are refused as ever
    r = binner("--fastq", fq, "-i", two, "-m", res, "--report", tmp_path / "rep.tsv")
    assert r.returncode == 1 and "index chunks" in r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--matched", tmp_path / "m")
    assert r.returncode == 1 and "index chunks" in r.stderr


def test_help_lists_the_switch():
    assert "--merge-on-gpu" in binner("--help").stdout
