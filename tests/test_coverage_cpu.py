"""CPU tests of coverage per reference: the restatement (cover_ref) against hand-computed cases, the host formatter against the
restatement's text, the table rules that need no device, the binner's usage errors, and the end-to-end condition on the
reference alone.  The table rules themselves are driven by tools/cover_refs_check.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cover_cases as CC
import cover_ref as R
import helpers
import mtsv_tools_amd as M
import pack_ref
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def rows_array(rows):
    a = np.zeros(len(rows), dtype=M.REF_COVERAGE_DTYPE)
    for k, name in enumerate(M.REF_COVERAGE_DTYPE.names):
        a[name] = [r[k] for r in rows]
    return a


# ---- the restatement ----

def test_the_restatement_on_hand_computed_cases():
    refs = [(5, 1, 100), (5, 2, 10), (9, 1, 64), (9, 1, 70), (9, 1, 3)]                 # the same reference thrice: the larger length
    recs = [(0, 5, 1, 0, 0), (0, 5, 1, 90, 0), (0, 5, 2, 9, 2),                         # read 0: two loci of one reference, one clamped
            (2, 5, 1, 20, 1), (2, 9, 1, 69, 1)]                                         # read 1 has no record
    read_len = [30, 50, 40]
    assert R.rows_of(refs, [(recs, read_len)]) == [(5, 1, 100, 2, 3, 30 + 10 + 40, 30 + 10 + 30), (5, 2, 10, 0, 0, 0, 0), (9, 1, 70, 1, 1, 1, 1)]
    assert R.rows_of(refs, [(recs, read_len)], 2)[1] == (5, 2, 10, 1, 1, 1, 1)
    assert R.rows_of(refs, [(recs, read_len)], 1) == R.rows_of(refs, [(recs, read_len)], 0)
    assert R.rows_of(refs, [(recs, read_len)], R.SLACK_ALL) == R.rows_of(refs, [(recs, read_len)], 2)
    # two calls: their reads are different reads, their positions the same positions
    twice = R.rows_of(refs, [(recs, read_len)] * 2)
    assert twice[0] == (5, 1, 100, 4, 6, 160, 70) and twice[2] == (9, 1, 70, 2, 2, 2, 1)
    for bad in ([(0, 5, 3, 0, 0)], [(0, 5, 2, 10, 0)], [(0, 9, 1, 70, 0)]):             # unknown; offset == L
        with pytest.raises(R.Refused):
            R.rows_of(refs, [(bad, read_len)])
    c = R.Coverage(refs)
    c.add_fold(recs, read_len)
    c.reset()
    assert c.rows() == R.rows_of(refs, [])


def test_the_restatement_on_the_edges_and_the_slack_case():
    refs, folds = CC.edges()
    rows = {(r[0], r[1]): r for r in R.rows_of(refs, folds)}
    assert rows[(5, 6)][6] == (256 - 63) + 130 + 520 + 7                               # [63, 256), [300, 430), [1000, 1520), [4090, 4097)
    assert rows[(6, 1)][3:] == (2, 2, 6, 5) and rows[(6, 2)][3:] == (0, 0, 0, 0)
    refs, folds = CC.slack()
    assert [r[3:5] for r in R.rows_of(refs, folds, 1)] == [(2, 3), (1, 1)]


# ---- the formatter ----

REPORT_ROWS = [
    (3, 1, 1000, 2, 3, 250, 200), (3, 2, 500, 0, 0, 0, 0), (3, 9, 3, 1, 1, 2, 2),       # a rollup over a reference without a hit
    (4, 1, 100, 0, 0, 0, 0), (4, 2, 100, 0, 0, 0, 0),                                   # a taxon without a hit prints nothing
    (6, 5, 0, 0, 0, 0, 0), (6, 6, 7, 1, 2, 14, 7),                                      # length 0 beside a hit
    (8, 1, 0, 1, 1, 0, 0),                                                              # hit, and of length 0: 0.00 for both
    (2 ** 31 + 7, 4, 3, 5, 5, 15, 3),                                                   # unsigned order
]


def test_format_coverage_report_is_the_restatements_text():
    text = M.format_coverage_report(rows_array(REPORT_ROWS))
    assert text == R.report(REPORT_ROWS)
    lines = text.decode().splitlines()
    assert lines[0].split("\t") == ["taxid", "gi", "length", "reads", "alignments", "aligned_bases", "depth", "covered_bases", "breadth_pct"]
    assert lines[1:] == [
        "3\t1\t1000\t2\t3\t250\t0.25\t200\t20.00", "3\t9\t3\t1\t1\t2\t0.67\t2\t66.67", "3\t*\t1503\t3\t4\t252\t0.17\t202\t13.44",
        "6\t6\t7\t1\t2\t14\t2.00\t7\t100.00", "6\t*\t7\t1\t2\t14\t2.00\t7\t100.00",
        "8\t1\t0\t1\t1\t0\t0.00\t0\t0.00", "8\t*\t0\t1\t1\t0\t0.00\t0\t0.00",
        "2147483655\t4\t3\t5\t5\t15\t5.00\t3\t100.00", "2147483655\t*\t3\t5\t5\t15\t5.00\t3\t100.00"]
    assert M.format_coverage_report(rows_array([])) == R.HEADER.encode() == R.report([])
    for refs, folds in (CC.edges(), CC.slack(), CC.random_case(seed=8, n_reads=150, n_refs=60)):
        rows = R.rows_of(refs, folds, 1)
        assert M.format_coverage_report(rows_array(rows)) == R.report(rows)


def test_the_abi_of_coverage():
    assert M.REF_COVERAGE_DTYPE.itemsize == 48
    L = M.lib()
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    for name in ("mtsv_coverage_create", "mtsv_coverage_free", "mtsv_coverage_add_index", "mtsv_coverage_add_refs", "mtsv_coverage_reset",
                 "mtsv_coverage_add_fold", "mtsv_coverage_rows", "mtsv_format_coverage_report"):
        assert name in src and name in _lib.EXPORTS and hasattr(L, name)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mtsv_format_coverage_report(None, 1, C.byref(out), C.byref(n)) == _lib.E_ARG
    assert L.mtsv_coverage_rows(None, C.byref(out), C.byref(n), None) == _lib.E_ARG
    assert L.mtsv_coverage_add_refs(None, None, None, None, 0) == _lib.E_ARG
    assert L.mtsv_coverage_reset(None) == _lib.E_ARG
    assert L.mtsv_coverage_add_fold(None, None, None, 0, 0, None) == _lib.E_ARG
    L.mtsv_coverage_free(None)


def test_create_without_a_device_fails_cleanly():
    if M.device_count() > 0:                                                            # with one, the table rules that need no kernel
        c = M.Coverage(0)
        c.add_refs([5, 5, 5], [1, 2, 1], [10, 0, 70])
        assert R.as_tuples(c.rows()[0]) == [(5, 1, 70, 0, 0, 0, 0), (5, 2, 0, 0, 0, 0, 0)]
        c.close()
        return
    h = C.c_void_p()
    assert M.lib().mtsv_coverage_create(0, C.byref(h)) == _lib.E_DEVICE and not h.value
    assert "no HIP device" in M.lib().mtsv_last_error().decode()
    with pytest.raises(M.MtsvError) as e:
        M.Coverage(0)
    assert e.value.code == _lib.E_DEVICE


# ---- the command line ----

def test_binner_usage_errors_of_coverage(tmp_path):
    base = ["--fastq", "x.fq", "-i", "a.idx,b.idx", "-m", str(tmp_path / "r")]
    cov = ["--coverage", str(tmp_path / "cov.tsv")]
    cases = [
        (cov + ["--output-format", "long"], "'--coverage <TSV>' requires '--fold-on-gpu'"),
        (cov + ["--fold-on-gpu"], "'--output-format long', or '--interleaved --pair-mode proper'"),
        (cov + ["--fold-on-gpu", "--interleaved", "--pair-mode", "both"], "'--output-format long', or '--interleaved --pair-mode proper'"),
        (["--fold-on-gpu", "--output-format", "long", "--coverage-slack", "1"], "'--coverage-slack <N|all>' requires '--coverage <TSV>'"),
        (cov + ["--fold-on-gpu", "--output-format", "long", "--coverage-slack", "some"], "Invalid value for '--coverage-slack <N>'"),
        (cov + ["--fold-on-gpu", "--output-format", "long", "--coverage-slack", "-1"], "Invalid value for '--coverage-slack <N>'"),
        (cov + ["--fold-on-gpu", "--output-format", "long", "--coverage-slack", "4294967296"], "Invalid value for '--coverage-slack <N>'"),
        (["--fold-on-gpu", "--output-format", "long", "--coverage"], "requires a value"),
    ]
    for args, message in cases:
        r = subprocess.run([BINNER, *base, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert not (tmp_path / "cov.tsv").exists()
    r = subprocess.run([BINNER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--coverage TSV [--coverage-slack N|all]" in r.stdout


# ---- the condition of the end-to-end test, on the reference alone ----

def test_the_reference_alone_covers_the_stretch_the_reads_were_cut_from(tmp_path):
    from oracle import oracle as O
    path = str(tmp_path / "chunk0.idx")
    M.MGIndex.synth(seed=5, n_taxa=8, gis_per_taxon=2, seq_len=20000).write(path)       # the first chunk of test_coverage.py
    index_file = pack_ref.IndexFile(path)
    b, s, e, reads = CC.tiled_reads(index_file)
    assert e - s >= 5000 and len(reads) == (e - s - CC.READ_LEN) // CC.STEP + 1
    bases, off = helpers.reads_to_batch(reads)
    hits, _ = O.Index.read(path).bin_batch(bases, off, O.default_params(), threads=8)
    recs = sorted(set((int(h["read"]), int(h["tax_id"]), int(h["gi"]), int(h["offset"]), int(h["edit"])) for h in hits))
    refs = [(x[1], x[0], x[3] - x[2]) for x in index_file.bins]
    rows = R.rows_of(refs, [(recs, [len(r) for r in reads])], 0)
    CC.condition(rows, b, s, e, CC.untouched_refs(index_file, b))
