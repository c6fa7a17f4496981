"""Taxa report, the parts that need no device: the semantics restated in Python (taxa_report_ref.py), the formatter
mtsv_format_taxa_report against hand-made rows and against bin/mtsv-collapse --report on the committed golden results,
the host-side merge of several workspaces' rows, and the command line's refusal of --report with a chunk list."""
import os
import subprocess

import numpy as np
import pytest

import mtsv_tools_amd as M
import taxa_report_ref as R
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
COLLAPSE = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
GOLD = os.path.join(ROOT, "tests", "golden")


def rows_of(*rows):
    out = np.zeros(len(rows), dtype=M.TAXON_STATS_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def test_restatement_on_hand_made_reads():
    # read 0: one taxon (twice: both strands) -> only_hit; read 1: a clear best; read 2: two tied and one worse;
    # read 3: the better edit of a taxon's two hits decides; read 5 has no hit (read 4 neither)
    hits = [(0, 7, 3), (0, 7, 1),
            (1, 7, 0), (1, 9, 2),
            (2, 7, 1), (2, 9, 1), (2, 4000000000, 5),
            (3, 9, 4), (3, 7, 3), (3, 9, 2)]
    read, tax, edit = (np.array(c) for c in zip(*hits))
    stats, total = R.classify(read, tax, edit)
    assert total == 4
    assert stats == {7: [1, 1, 1, 1], 9: [0, 1, 1, 1], 4000000000: [0, 0, 0, 1]}
    # the order of the hits does not matter
    p = np.random.default_rng(1).permutation(len(hits))
    assert R.classify(read[p], tax[p], edit[p]) == (stats, total)
    assert R.classify(np.zeros(0), np.zeros(0), np.zeros(0)) == ({}, 0)


def test_struct_layout():
    assert M.TAXON_STATS_DTYPE.itemsize == 40
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    assert "uint64_t only_hit, only_best, tied_best, not_best;" in src


def test_formatter_on_hand_made_rows():
    # percentages that need rounding: 1 of 3, 2 of 3
    got = M.format_taxa_report(rows_of((5, 1, 0, 2, 0), (4000000000, 0, 1, 0, 2)), 3)
    assert got == (R.HEADER
                   + "5\t1\t33.33\t0\t0.00\t2\t66.67\t0\t0.00\t3\t100.00\n"
                   + "4000000000\t0\t0.00\t1\t33.33\t0\t0.00\t2\t66.67\t3\t100.00\n").encode()
    # 1 of 7; a row's sum may exceed total_reads only in hand-made input, the formatter does not care
    got = M.format_taxa_report(rows_of((1, 1, 2, 3, 4)), 7)
    assert got == (R.HEADER + "1\t1\t14.29\t2\t28.57\t3\t42.86\t4\t57.14\t10\t142.86\n").encode()
    # total_reads == 0: the denominator is max(total_reads, 1)
    assert M.format_taxa_report(rows_of((9, 0, 0, 0, 0)), 0) == (R.HEADER + "9\t0\t0.00\t0\t0.00\t0\t0.00\t0\t0.00\t0\t0.00\n").encode()
    assert M.format_taxa_report(rows_of((9, 2, 0, 0, 0)), 0) == (R.HEADER + "9\t2\t200.00\t0\t0.00\t0\t0.00\t0\t0.00\t2\t200.00\n").encode()
    assert M.format_taxa_report(rows_of(), 12) == R.HEADER.encode()
    # counters above 2^32
    big = (1 << 32) + 5
    got = M.format_taxa_report(rows_of((2147483649, big, 0, 0, big)), 4 * big)
    assert got == (R.HEADER + f"2147483649\t{big}\t25.00\t0\t0.00\t0\t0.00\t{big}\t25.00\t{2 * big}\t50.00\n").encode()


def collapse_report(tmp_path, results_path):
    out, rep = tmp_path / "collapsed.txt", tmp_path / "collapse_report.tsv"
    r = subprocess.run([COLLAPSE, "-o", str(out), "--report", str(rep), str(results_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return rep.read_bytes()


def test_formatter_prints_a_binary_tie_as_the_collapse_tool_does(tmp_path):
    """1 of 32 = 3.125 exactly: only required to come out as bin/mtsv-collapse --report writes it (%.2f); how the
    reference's {:.2} prints an exact tie is not settled here"""
    res = tmp_path / "tie.results"
    res.write_text("".join(f"r{i}:{5 if i == 0 else 6}=0\n" for i in range(32)))
    want = collapse_report(tmp_path, res)
    assert M.format_taxa_report(rows_of((5, 1, 0, 0, 0), (6, 31, 0, 0, 0)), 32) == want


@pytest.mark.parametrize("name,sums", [("e2e_default", (74, 24, 117, 358)), ("e2e_stress", (52, 0, 0, 0))])
def test_formatter_and_restatement_against_collapse_on_golden_results(tmp_path, name, sums):
    path = os.path.join(GOLD, f"{name}.results")
    want = collapse_report(tmp_path, path)
    rows = R.parse_report(want.decode())
    ids, read, tax, edit = R.parse_results(open(path).read())
    assert len(set(ids)) == len(ids)          # unique IDs: the tool's per-ID merge and the per-read count agree
    stats, total = R.classify(read, tax, edit)
    assert total == len(ids)
    assert stats == rows
    assert tuple(sum(r[c] for r in rows.values()) for c in range(4)) == sums
    if name == "e2e_default":
        assert (len(ids), len(rows)) == (140, 12)
        assert rows[2] == [38, 5, 10, 50] and rows[4000000000] == [5, 0, 0, 0]
    assert M.format_taxa_report(R.rows_array(rows, M.TAXON_STATS_DTYPE), total) == want


def test_merge_of_two_workspaces_rows():
    a = rows_of((2, 1, 0, 0, 0), (9, 0, 1, 2, 3), (4000000000, 1 << 33, 0, 0, 0))
    b = rows_of((1, 0, 0, 0, 7), (9, 5, 5, 5, 5), (4000000000, 1, 0, 0, 0))
    got = M.merge_taxa_reports(a, b)
    assert R.rows_dict(got) == {1: [0, 0, 0, 7], 2: [1, 0, 0, 0], 9: [5, 6, 7, 8], 4000000000: [(1 << 33) + 1, 0, 0, 0]}
    assert list(got["tax_id"]) == [1, 2, 9, 4000000000]
    assert len(M.merge_taxa_reports(rows_of(), rows_of())) == 0
    assert R.rows_dict(M.merge_taxa_reports(a, rows_of())) == R.rows_dict(a)
    with pytest.raises(M.MtsvError) as e:
        M.merge_taxa_reports(rows_of((9, 1, 0, 0, 0), (2, 1, 0, 0, 0)), b)
    assert e.value.code == _lib.E_ARG


def test_cli_refuses_report_with_a_chunk_list_and_lists_the_flag(tmp_path):
    res, rep = tmp_path / "r.txt", tmp_path / "rep.tsv"
    r = subprocess.run([BINNER, "--fasta", "x", "-i", "a.idx,b.idx", "-m", str(res), "--report", str(rep)], capture_output=True, text=True)
    assert r.returncode != 0
    assert "mtsv-collapse --report" in r.stderr
    assert not res.exists() and not rep.exists()      # refused before anything is opened
    r = subprocess.run([BINNER, "--fasta", "x", "--index=a.idx,b.idx", "--report=" + str(rep), "-m", str(res)], capture_output=True, text=True)
    assert r.returncode != 0 and "mtsv-collapse --report" in r.stderr
    assert subprocess.run([BINNER, "--fasta", "x", "-i", "y", "-m", str(res), "--report"], capture_output=True).returncode == 1
    h = subprocess.run([BINNER, "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and "--report" in h.stdout
