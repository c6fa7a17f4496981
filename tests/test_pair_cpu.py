"""CPU-side tests of the pair join: the restatement (pair_ref) on hand-written cases, the exported symbol, and the refusals of
mtsv-binner --interleaved that are decided before a device is touched.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import mtsv_tools_amd as M
import pair_cases as PC
import pair_ref as R
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


# ---- the restatement ----

def test_both_sums_the_mates_smallest_edits():
    recs = [(0, 5, 3), (0, 7, 1), (1, 5, 2), (1, 9, 0),              # pair 0: only 5 is shared
            (2, 5, 1), (5, 5, 1),                                    # pairs 1 and 2: one mate each
            (6, 4, 2), (6, 8, 0), (7, 4, 0), (7, 8, 4)]
    assert R.pair(R.BOTH, recs) == [(0, 5, 5), (3, 4, 2), (3, 8, 4)]
    assert R.stats(recs, 8, R.pair(R.BOTH, recs)) == {"pairs": 4, "both_mates_hit": 2, "one_mate_hit": 2, "joined": 2, "records": 3}
    # at a wide grain a TaxID has several records per mate: the smallest of each
    wide = [(0, 5, 1, 10, 4), (0, 5, 2, 10, 2), (1, 5, 1, 900, 1), (1, 5, 3, 0, 3)]
    assert R.pair(R.BOTH, wide) == [(0, 5, 3)]


def test_either_prices_the_mate_that_did_not_align():
    recs = [(0, 5, 3), (0, 7, 1), (1, 5, 2), (1, 9, 0), (2, 5, 1), (5, 5, 1)]
    assert R.pair(R.EITHER, recs, unpaired_edits=10) == [(0, 5, 5), (0, 7, 11), (0, 9, 10), (1, 5, 11), (2, 5, 11)]
    assert R.pair(R.EITHER, recs, unpaired_edits=0) == [(0, 5, 5), (0, 7, 1), (0, 9, 0), (1, 5, 1), (2, 5, 1)]
    # max_insert is ignored
    assert R.pair(R.EITHER, recs, max_insert=7, unpaired_edits=10) == R.pair(R.EITHER, recs, unpaired_edits=10)


def test_proper_takes_the_smallest_sum_not_the_best_record_and_its_nearest():
    # mate 0's best record (edit 0, offset 100) has only an edit-9 partner in reach; the couple (edit 2 at 5000, edit 1 at 5100)
    # sums to 3
    recs = [(0, 5, 1, 100, 0), (0, 5, 1, 5000, 2), (1, 5, 1, 150, 9), (1, 5, 1, 5100, 1), (1, 5, 1, 9000, 0)]
    assert R.pair(R.PROPER, recs, max_insert=300) == [(0, 5, 3)]
    assert R.pair(R.BOTH, recs) == [(0, 5, 0)]
    assert R.pair(R.PROPER, recs, max_insert=49) == []


def test_proper_needs_the_same_gi():
    recs = [(0, 5, 1, 100, 0), (1, 5, 2, 100, 0), (2, 6, 4, 0, 1), (3, 6, 4, 0, 2)]
    assert R.pair(R.BOTH, recs) == [(0, 5, 0), (1, 6, 3)]
    assert R.pair(R.PROPER, recs, max_insert=1000) == [(1, 6, 3)]


def test_proper_window_edges_in_both_directions():
    for d, kept in ((300, True), (301, False)):
        ahead = [(0, 5, 1, 1000, 1), (1, 5, 1, 1000 + d, 1)]
        behind = [(0, 5, 1, 1000 + d, 1), (1, 5, 1, 1000, 1)]
        for recs in (ahead, behind):
            assert R.pair(R.PROPER, recs, max_insert=300) == ([(0, 5, 2)] if kept else [])
    # no wrap at either end of the offsets
    n_reads, recs = PC.offsets()
    assert R.pair(R.PROPER, recs, max_insert=0) == [(3, 7, 7), (4, 7, 7)]
    assert R.pair(R.PROPER, recs, max_insert=1) == [(0, 7, 2), (3, 7, 7), (4, 7, 7)]
    assert R.pair(R.PROPER, recs, max_insert=2 ** 32 - 1) == [(0, 7, 2), (1, 7, 0), (2, 7, 0), (3, 7, 7), (4, 7, 7)]


def test_pair_ids():
    assert R.stem("frag7", "frag7") == "frag7" and R.stem("frag7/1", "frag7/2") == "frag7"
    assert R.stem("frag7/2", "frag7/1") is None and R.stem("a/1", "b/2") is None and R.stem("a", "b") is None
    assert R.lines([(0, 5, 1), (0, 9, 0), (2, 4, 7)], ["p0", "p1", "p2"]) == b"p0:5=1,9=0\np2:4=7\n"


def test_cases_are_lists_of_their_grains():
    import fold_ref as F
    import random
    for n_reads, wide in (PC.edges(), PC.offsets(), PC.windows(), PC.straddle(), PC.heavy(64, 4), PC.random_pairs(random.Random(1), 50)):
        for grain in PC.GRAINS.values():
            recs = PC.project(grain, wide)
            assert F.is_list(grain, recs) and all(r[0] < n_reads for r in recs) and n_reads % 2 == 0
    assert PC.project(F.LONG, PC.straddle()[1])[63][:2] == (0, 2)     # record 63, the last of the first tile of 64, is a head


# ---- the library ----

def test_symbol_constants_and_null_handles():
    L = M.lib()
    assert hasattr(L, "mtsv_fold_pair") and "mtsv_fold_pair" in _lib.EXPORTS
    assert (M.PAIR_BOTH, M.PAIR_EITHER, M.PAIR_PROPER) == (0, 1, 2) == (R.BOTH, R.EITHER, R.PROPER)
    assert C.sizeof(M.PairStats) == 40
    st = M.PairStats()
    assert L.mtsv_fold_pair(None, M.PAIR_BOTH, 0, 0, None, C.byref(st), None) == _lib.E_ARG
    assert b"null" in L.mtsv_last_error()


# ---- the command line: what resolve() refuses before a device is touched ----

def binner(tmp_path, *args):
    fq = tmp_path / "in.fasta"
    fq.write_text(">a/1\nACGT\n>a/2\nACGT\n")
    r = subprocess.run([BINNER, "--fasta", str(fq), "-i", "a.idx,b.idx", "-m", str(tmp_path / "out.res"), *args], capture_output=True, text=True,
                       timeout=120)
    assert not (tmp_path / "out.res").exists() or (tmp_path / "out.res").read_text() == "kept\n"
    return r


def test_cli_refusals(tmp_path):
    def refused(*args):
        r = binner(tmp_path, *args)
        assert r.returncode == 1 and r.stderr.startswith("error: "), (args, r.returncode, r.stderr)
        return r.stderr

    assert "'--interleaved' requires '--fold-on-gpu'" in refused("--interleaved")
    assert "'--interleaved' cannot be used with '--output-format long'" in refused("--interleaved", "--fold-on-gpu", "--output-format", "long")
    assert "'--interleaved' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'" in refused("--interleaved", "--fold-on-gpu", "--matched", str(tmp_path / "m"))
    assert "'--interleaved' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'" in refused("--interleaved", "--fold-on-gpu", "--unmatched", str(tmp_path / "u"))
    assert "'--interleaved' cannot be used with '--filter-index <INDEX>'" in refused("--interleaved", "--fold-on-gpu", "--filter-index", "f.idx")
    assert "'--pair-mode either' requires '--unpaired-penalty <N>'" in refused("--interleaved", "--fold-on-gpu", "--pair-mode", "either")
    assert "isn't a valid value for '--pair-mode <MODE>'" in refused("--interleaved", "--fold-on-gpu", "--pair-mode", "improper")
    assert "Invalid value for '--max-insert <N>'" in refused("--interleaved", "--fold-on-gpu", "--max-insert", "4294967296")
    assert "needs an even '--read-offset'" in refused("--interleaved", "--fold-on-gpu", "--read-offset", "3")
    for flag, value in (("--pair-mode", "both"), ("--max-insert", "5"), ("--unpaired-penalty", "5")):
        assert f"requires '--interleaved'" in refused("--fold-on-gpu", flag, value)
    # an existing results file would be resumed
    (tmp_path / "out.res").write_text("kept\n")
    assert "'--interleaved' does not resume" in refused("--interleaved", "--fold-on-gpu")
    (tmp_path / "out.res").unlink()


def test_help_names_the_flags():
    r = subprocess.run([BINNER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for word in ("--interleaved", "--pair-mode both|either|proper", "--max-insert", "--unpaired-penalty"):
        assert word in r.stdout
