"""What of the fold needs no GPU: the restatement (fold_ref.py) against the collapse of the merged hits on the chunked
fixtures, in every grain and folding order; the report and the flags derived from records; the library's exports, a fold on a
device that does not exist, and the argument rules of mtsv-binner --fold-on-gpu, which are decided before any index is opened.

Expected values come from the CPU oracle's hits through the restatements of the collapse (assign_ref.py, grain_ref.py), the
merge (chunk_merge_ref.py) and the report (taxa_report_ref.py)."""
import ctypes
import os
import re
import subprocess

import pytest

import assign_ref as A
import chunk_merge_ref as CM
import fold_ref as F
import grain_cases as G
import grain_ref as GR
import helpers
import mtsv_tools_amd as M
import taxa_report_ref as R
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_chunk_merge import make_planted5, make_tricky3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
COLLAPSE = {F.TAXID: A.collapse, F.LONG: GR.collapse_long, F.TAXID_GI: GR.collapse_taxid_gi}
FOLD_SYMBOLS = ("mtsv_fold_create", "mtsv_fold_free", "mtsv_fold_reset", "mtsv_fold_add_run", "mtsv_fold_add_records", "mtsv_fold_count",
                "mtsv_fold_download", "mtsv_fold_download_gi", "mtsv_fold_taxa_report", "mtsv_fold_match_flags")


def grain_parts():
    first, second, seg, half, rng = G.database()
    reads = G.reads(rng, seg, half, first, n_seg=12, n_pal=6, n_bg=12)
    bases, off = helpers.reads_to_batch(reads)
    return [O.Index.build(e).bin_batch(bases, off, O.default_params(), threads=8)[0] for e in (first, second)], len(reads)


@pytest.fixture(scope="module", params=["tricky3", "planted5", "grain_cases"])
def chunked(request):
    """(per-chunk hit lists, their merge, number of reads)"""
    if request.param == "grain_cases":
        parts, n = grain_parts()
    else:
        fx = make_tricky3() if request.param == "tricky3" else make_planted5()
        parts, n = fx.parts(), fx.n
    return parts, CM.merge_hits(parts), n


@pytest.mark.parametrize("grain", [F.TAXID, F.LONG, F.TAXID_GI], ids=["taxid", "long", "taxid_gi"])
def test_fold_of_the_chunk_collapses_is_the_collapse_of_the_merge(chunked, grain):
    parts, merged, n = chunked
    lists = [COLLAPSE[grain](p) for p in parts]
    want = COLLAPSE[grain](merged)
    assert len(want) > 0 and all(F.is_list(grain, l) for l in lists) and F.is_list(grain, want)
    if grain == F.TAXID:
        assert sum(len(l) for l in lists) > len(want)                          # keys that two chunks hold
    assert F.fold_all(grain, lists) == want                                    # chunk order
    assert F.fold_all(grain, lists[::-1]) == want                              # reversed
    tree = F.fold(grain, F.fold(grain, lists[0], lists[1]), F.fold_all(grain, lists[2:]))
    assert tree == want                                                        # (0 + 1) + (2 + ..)
    # what is counted per read, from the records alone
    assert F.report(want) == R.classify_hits(merged)
    pres = CM.presence(merged, n)
    assert F.flags(want, n).tolist() == pres.tolist() and F.report(want)[1] == int(pres.sum())


def test_restatement_on_hand_made_lists():
    B = 1 << 31
    a = [(0, 7, 3), (0, B + 1, 2), (2, 5, 9)]
    b = [(0, 7, 1), (1, 4, 4), (2, 5, 9), (2, B, 0)]
    assert F.fold(F.TAXID, a, b) == [(0, 7, 1), (0, B + 1, 2), (1, 4, 4), (2, 5, 9), (2, B, 0)]
    assert F.fold(F.TAXID, b, a) == F.fold(F.TAXID, a, b) and F.fold(F.TAXID, a, []) == a and F.fold(F.TAXID, [], []) == []
    # TAXID_GI: equal edits, the smaller offset wins; a smaller edit wins whatever its offset
    ga = [(0, 7, 1, 9, 3), (0, 7, 2, 50, 2)]
    gb = [(0, 7, 1, 4, 3), (0, 7, 2, 1, 5)]
    assert F.fold(F.TAXID_GI, ga, gb) == [(0, 7, 1, 4, 3), (0, 7, 2, 50, 2)]
    # LONG: the offset is part of the key
    assert F.fold(F.LONG, ga, gb) == [(0, 7, 1, 4, 3), (0, 7, 1, 9, 3), (0, 7, 2, 1, 5), (0, 7, 2, 50, 2)]
    stats, total = F.report([(0, 7, 1, 4, 3), (0, 7, 2, 50, 2), (0, 9, 1, 0, 2), (3, 9, 1, 0, 8)])
    assert total == 2 and stats == {7: [0, 0, 1, 0], 9: [1, 0, 1, 0]}
    assert F.flags([(0, 7, 1), (3, 9, 8)], 5).tolist() == [True, False, False, True, False]


def test_library_exports_every_fold_symbol():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.lib_path())
    for name in FOLD_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert "typedef struct mtsv_fold mtsv_fold;" in src and hasattr(M, "Fold")


def test_fold_on_a_device_that_does_not_exist_is_a_device_error():
    with pytest.raises(M.MtsvError) as e:
        M.Fold(M.device_count(), M.GRAIN_TAXID)                                # the first ordinal that is not there
    assert e.value.code == _lib.E_DEVICE
    with pytest.raises(M.MtsvError) as e:
        M.Fold(M.device_count(), 7)                                            # a bad grain is an argument error first
    assert e.value.code == _lib.E_ARG


def test_record_checks_of_add_records_under_the_sanitizers(tmp_path):
    """the host-side checks of mtsv_fold_add_records (csrc/fold_records.hpp) as a stand-alone program, built with the address
    and undefined-behaviour sanitizers and run on the CPU"""
    exe = tmp_path / "fold_records_check"
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tools", "fold_records_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "fold_records_check ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def binner(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_fold_on_gpu_argument_rules_are_decided_before_any_index_is_opened(tmp_path):
    """every run names index files that do not exist: a run that got as far as loading one would exit 2"""
    res, fq = tmp_path / "res", tmp_path / "x.fastq"
    two = f"{tmp_path}/a.idx,{tmp_path}/b.idx"
    r = binner("--fastq", fq, "-i", tmp_path / "a.idx", "-m", res, "--fold-on-gpu")
    assert r.returncode == 1 and "--fold-on-gpu" in r.stderr and "chunks" in r.stderr
    r = binner("--fastq", fq, "-i", f"{tmp_path}/a.idx,", "-m", res, "--fold-on-gpu")            # one entry and a comma
    assert r.returncode == 1 and "--fold-on-gpu" in r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--devices", "0,1")
    assert r.returncode == 1 and "--fold-on-gpu" in r.stderr and "--devices" in r.stderr
    for other in (["--merge-on-gpu"], ["--filter-index", tmp_path / "f.idx"], ["--parse-only"]):
        r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", *other)
        assert r.returncode == 1 and "--fold-on-gpu" in r.stderr and str(other[0]) in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--fold-reads", "0")
    assert r.returncode == 1 and "--fold-reads" in r.stderr
    assert not res.exists()
    # a results file that the run would resume
    res.write_text("r0:7=1\n")
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu")
    assert r.returncode == 1 and "--fold-on-gpu" in r.stderr and "resume" in r.stderr
    assert res.read_text() == "r0:7=1\n"
    res.unlink()
    # with a proper chunk list the report and the partition files are accepted: the run gets as far as its input
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--report", tmp_path / "rep.tsv", "--matched", tmp_path / "m")
    assert r.returncode == 2, r.stderr
    r = binner("--fastq", fq, "-i", two, "--fold-on-gpu", "--unmatched", tmp_path / "u", "--devices", "0", "--fold-reads", "100")
    assert r.returncode == 2, r.stderr


def test_help_lists_the_switch():
    out = binner("--help").stdout
    assert "--fold-on-gpu" in out and "--fold-reads" in out
