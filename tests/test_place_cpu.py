"""CPU tests of the alignments of hits (mtsv_batch_place_hits, mtsv_format_placements, mtsv-binner --alignments): the
restatement place_ref pinned to the oracle's edit distance and to the definition of its own edit scripts, the crafted cases
of test_place.py against what they are meant to reach, the formatter, the ABI."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import place_cases as PC
import place_ref as R
from mtsv_tools_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
LETTER = b"ACGTN"


def as_bytes(code_array, n_as):
    """codes as the bytes the oracle compares: an N of the read is '.', which equals nothing in a text (align.rs)"""
    return bytes(n_as if c >= 4 else LETTER[c] for c in code_array)


def seeded_pairs(n=2000, seed=23):
    rng = random.Random(seed)
    for k in range(n):
        L = 1 + (k * 7919) % 256                                                         # every length 1..256, several times
        text = helpers.rnd_seq(rng, L + rng.randrange(0, 90), b"ACGTN" if k % 3 == 0 else b"ACGT")
        at = rng.randrange(0, max(1, len(text) - L + 1))
        P = helpers.mutate(rng, text[at:at + L], rng.randrange(0, int(0.45 * L) + 1), b"ACGTN" if k % 4 == 0 else b"ACGT")
        P = (P + helpers.rnd_seq(rng, L))[:L]
        strand = k & 1
        yield (helpers.revcomp(P) if strand else P), strand, text


def test_the_restatement_against_the_oracle_and_its_own_scripts():
    lengths = set()
    for read, strand, text in seeded_pairs():
        P, T = R.strand_codes(read, strand), R.codes(text)
        assert strand == 0 or bytes(as_bytes(P, ord("N"))) == helpers.revcomp(read)
        pb, tb = as_bytes(P, ord(".")), as_bytes(T, ord("N"))
        m = O.min_edit_distance(pb, tb)
        assert R.min_edit(P, T) == m
        got = R.place(P, T, m)
        assert got is not None and got.cost == m
        # the leftmost column that reaches m: the window up to any end at or behind it has the same minimum, a shorter one a larger
        for end in {got.end, (got.end + len(T) + 1) // 2, len(T)}:
            assert O.min_edit_distance(pb, tb[:end]) == m
        assert got.end == 0 or O.min_edit_distance(pb, tb[:got.end - 1]) > m
        R.check_cigar(P, T, got, m)
        assert sum(n for n, op in got.ops if op != R.OP_EQ) == m
        assert R.place(P, T, m - 1) is None                                               # one below the minimum: unplaceable
        lengths.add(len(P))
    assert lengths == set(range(1, 257))


def test_an_edit_of_the_reads_length_or_more_ends_at_column_zero():
    P, T = R.codes(b"ACGTA"), R.codes(b"ACGTAGG")
    for edit in (5, 6, 0xffffffff):
        assert R.place(P, T, edit) == R.Placed(0, 0, 5, [(5, R.OP_I)])
    assert R.place(P, T, 4).end == 1 and R.place(P, T, 0) == R.Placed(0, 5, 0, [(5, R.OP_EQ)])
    assert R.place(R.codes(b""), T, 0) == R.Placed(0, 0, 0, [])
    assert R.place(R.codes(b"N"), R.codes(b"N"), 0) is None                               # an N over an N is no match
    assert R.place(R.codes(b"ANA"), R.codes(b"GGANAG"), 1) == R.Placed(2, 5, 1, [(1, R.OP_EQ), (1, R.OP_X), (1, R.OP_EQ)])


@pytest.fixture(scope="module")
def crafted():
    entries = PC.database()
    reads, hits = PC.crafted(entries)
    return entries, reads, hits, PC.expected(entries, reads, hits)


def test_the_crafted_cases_reach_what_they_are_meant_to(crafted):
    entries, reads, hits, want = crafted
    text_of = {(t, g): s for t, g, s in entries}
    assert len(hits) >= 200 and all(w is not None for w in want)
    assert {len(r) for r in reads} == set(PC.LENGTHS) and {h[5] for h in hits} == {0, 1}
    seen = set()
    for (r, t, g, o, e, strand), (start, end, ops) in zip(hits, want):
        P, T = R.strand_codes(reads[r], strand), R.codes(text_of[(t, g)][o:])
        R.check_cigar(P, T, R.Placed(start - o, end - o, sum(n for n, op in ops if op != R.OP_EQ), ops), e)
        L = len(P)
        reached = {"start0": start == o, "one_in": start == o + 1, "far": start - o >= PC.FAR - 1,
                   "bin_end": end == PC.BIN_LEN and (t, g) != (3, 30), "text_end": end == PC.BIN_LEN and (t, g) == (3, 30),
                   "text_begin": (t, g) == (1, 10) and o == 0, "n_over_n": bool((P == 4).any())}
        seen.update((what, L) for what, yes in reached.items() if yes)
        seen.update((op, L) for n, op in ops)
        if reached["n_over_n"] and L >= 31 and e <= 3:                                    # the read's N over the text's N: an X each
            per_base = [op for n, op in ops for _ in range(n) if op != R.OP_D]
            assert [per_base[i] for i in np.nonzero(P == 4)[0]] == [R.OP_X, R.OP_X]
    for L in PC.LENGTHS:
        if L >= 31:                                                                       # (a read of one base matches wherever it likes)
            for what in ("start0", "one_in", "far", "bin_end", "text_end", "text_begin", "n_over_n", R.OP_I, R.OP_D, R.OP_X, R.OP_EQ):
                assert (what, L) in seen, (what, L)
    assert max(e for _, _, _, _, e, _ in hits) > int(0.13 * 256)                          # heavier than a default run accepts


# ---- the formatter ----

def placements(rows):
    """rows: (read, tax_id, gi, strand, start, end, edit, ops) -> (PLACEMENT_DTYPE array, ops array with a gap before every script)"""
    pl = np.zeros(len(rows), dtype=M.PLACEMENT_DTYPE)
    flat = []
    for k, (read, t, g, strand, start, end, edit, ops) in enumerate(rows):
        flat += [0xdead0] * (k % 3)                                                       # unused slots between hits
        pl[k] = (read, t, g, edit, strand, start, end, len(ops), len(flat))
        flat += R.encode(ops)
    return pl, np.array(flat, dtype=np.uint32)


FORMAT_ROWS = [
    (0, 9, 1000, 0, 5, 155, 0, [(150, R.OP_EQ)]),                                         # edit 0
    (1, 9, 1000, 1, 0, 0, 7, [(7, R.OP_I)]),                                              # all I: no reference base
    (2, 4000000000, 4294967295, 0, 4294967000, 4294967295, 3, [(2, R.OP_D), (37, R.OP_EQ), (1, R.OP_X), (112, R.OP_EQ)]),  # a leading D
    (1, 2, 5, 1, 10, 13, 1, [(1, R.OP_EQ), (1, R.OP_I), (1, R.OP_X), (1, R.OP_D), (1, R.OP_EQ)]),
    (3, 2, 5, 0, 17, 17, 0, []),                                                          # a read of no bases
]
IDS = ["r0", "read/1 with a space", "", "last"]


def test_format_placements_is_the_restatements_text():
    pl, ops = placements(FORMAT_ROWS)
    want = "".join(R.line(IDS[r], t, g, s, a, b, e, o) for r, t, g, s, a, b, e, o in FORMAT_ROWS)
    assert M.format_placements(pl, ops, IDS) == want
    assert "\t+\t5\t155\t0\t150=\n" in want and "\t7I\n" in want and "\t2D37=1X112=\n" in want and want.endswith("\t17\t17\t0\t*\n")
    assert M.format_placements(pl[:0], ops[:0], IDS) == ""
    for k in range(len(pl)):                                                              # any order, any subset
        assert M.format_placements(pl[k:k + 1], ops, IDS) == R.line(IDS[FORMAT_ROWS[k][0]], *FORMAT_ROWS[k][1:])
    bad = pl.copy()
    bad["read"][2] = len(IDS)                                                             # a read number out of range
    with pytest.raises(M.MtsvError) as e:
        M.format_placements(bad, ops, IDS)
    assert e.value.code == _lib.E_ARG and "read 4" in str(e.value)


def test_the_abi_of_placements():
    assert M.PLACEMENT_DTYPE.itemsize == 48 and M.PLACEMENT_DTYPE.fields["ops_off"][1] == 40
    assert (M.CIGAR_I, M.CIGAR_D, M.CIGAR_EQ, M.CIGAR_X) == (R.OP_I, R.OP_D, R.OP_EQ, R.OP_X) == (1, 2, 7, 8)
    L = M.lib()
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    for name in ("mtsv_batch_place_hits", "mtsv_format_placements", "mtsv_placement"):
        assert name in src
    for name in ("mtsv_batch_place_hits", "mtsv_format_placements"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    out, n, ops, n_ops = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    assert L.mtsv_batch_place_hits(None, None, 0, C.byref(out), C.byref(n), C.byref(ops), C.byref(n_ops), None) == _lib.E_ARG
    assert L.mtsv_format_placements(None, 1, None, b"", None, 0, C.byref(out), C.byref(n)) == _lib.E_ARG


# ---- the command line ----

def test_binner_usage_errors_of_alignments(tmp_path):
    base = ["--fastq", "x.fq", "-i", "a.idx,b.idx", "-m", str(tmp_path / "r")]
    aln = ["--alignments", str(tmp_path / "aln.tsv")]
    cases = [
        (aln, "'--alignments <FILE>' requires '--fold-on-gpu'"),
        (aln + ["--merge-on-gpu"], "'--alignments <FILE>' requires '--fold-on-gpu'"),
        (aln + ["--fold-on-gpu", "--dedup"], "'--alignments <FILE>' cannot be used with '--dedup': only the representatives"),
        (["--alignments", str(tmp_path / "r"), "--fold-on-gpu"], "'--alignments <FILE>' and '-m/--results <RESULTS>' name the same file"),
        (["--fold-on-gpu", "--alignments"], "requires a value"),
    ]
    for args, message in cases:
        r = subprocess.run([BINNER, *base, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert "USAGE" not in r.stderr or "requires a value" in message                   # a refusal prints no usage text
        assert not (tmp_path / "aln.tsv").exists() and not (tmp_path / "r").exists()
    r = subprocess.run([BINNER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--alignments FILE (only with --fold-on-gpu, not with --dedup" in r.stdout
