"""Assignments, the parts that need no device: the semantics restated in Python (assign_ref.py) against the oracle's
own result lines, the formatter mtsv_format_assignments against mtsv_format_results, the refusals, the struct."""
import os
import random

import numpy as np
import pytest

import assign_cases as K
import assign_ref as A
import helpers
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hits_of(rows):
    """(read, tax_id, gi, edit, strand, offset) rows as a HIT_DTYPE array"""
    out = np.zeros(len(rows), dtype=M.HIT_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def test_struct_layout():
    assert M.ASSIGN_DTYPE.itemsize == 16
    assert [M.ASSIGN_DTYPE.fields[f][1] for f in ("read", "tax_id", "edit")] == [0, 8, 12]
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    assert "} mtsv_assignment;" in src
    assert (M.ASSIGN_OFF, M.ASSIGN_WITH_HITS, M.ASSIGN_ONLY) == (0, 1, 2)


def test_restatement_on_hand_made_hits():
    hits = hits_of([(0, 7, 1, 3, 0, 10), (0, 7, 2, 1, 1, 20),                       # the smaller edit comes second
                    (1, 9, 1, 2, 0, 1), (1, 7, 1, 0, 0, 2), (1, 9, 3, 2, 1, 3),     # equal edits twice
                    (3, 4000000000, 1, 5, 0, 1), (3, 3, 1, 9, 0, 1), (3, 2147483648, 1, 0, 1, 4), (3, 3, 2, 4, 1, 9)])
    want = [(0, 7, 1), (1, 7, 0), (1, 9, 2), (3, 3, 4), (3, 2147483648, 0), (3, 4000000000, 5)]
    assert A.collapse(hits) == want
    p = np.random.default_rng(3).permutation(len(hits))
    assert A.collapse(hits[p]) == want                    # the order of the hits does not matter
    assert A.collapse(hits[:0]) == []
    ids = ["a", "b", "c", "d"]
    assert A.text(want, ids) == "a:7=1\nb:7=0,9=2\nd:3=4,2147483648=0,4000000000=5\n"
    assert A.as_triples(A.as_array(want, M.ASSIGN_DTYPE)) == want


def test_restatement_against_the_oracle_lines_on_the_tricky_database(tmp_path):
    entries, gene, unit = helpers.tricky_db(seed=7)
    orc = O.Index.build(entries)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=12, lengths=(150,))
    bases, off = helpers.reads_to_batch(reads)
    hits, _ = orc.bin_batch(bases, off, O.default_params(), threads=8)
    ids = [f"R{i}" for i in range(len(reads))]
    want = "".join(O.format_line(ids[r], hits[hits["read"] == r]) for r in sorted(set(hits["read"].tolist())))
    got = A.collapse(hits)
    assert A.text(got, ids) == want
    assert M.format_assignments(A.as_array(got, M.ASSIGN_DTYPE), ids) == want
    assert M.format_results(hits, ids) == want


def test_restatement_against_the_oracle_lines_where_taxa_repeat():
    """the tier database of the device tests: every read has about 120 hits on 90 TaxIDs"""
    entries, seg, rng = K.tier_db()
    orc = O.Index.build(entries)
    reads = K.tier_reads(rng, seg, 24)
    bases, off = helpers.reads_to_batch(reads)
    hits, _ = orc.bin_batch(bases, off, O.default_params(), threads=8)
    diff, later, same = K.duplicate_census(hits)
    assert diff and later and same and later < diff
    ids = [f"R{i}" for i in range(len(reads))]
    want = "".join(O.format_line(ids[r], hits[hits["read"] == r]) for r in sorted(set(hits["read"].tolist())))
    got = A.collapse(hits)
    assert len(got) == 90 * len(reads) < len(hits)
    assert A.text(got, ids) == want
    assert M.format_assignments(A.as_array(got, M.ASSIGN_DTYPE), ids) == want


def test_formatter_equals_format_results_on_hand_made_hits():
    rng = random.Random(5)
    rows = []
    # read 0: the largest TaxID and ten-digit edits; read 2: 3000 TaxIDs, most of them twice, in random order
    rows += [(0, 4294967295, 1, 4294967295, 0, 0), (0, 4294967295, 2, 4000000000, 1, 0), (0, 0, 1, 1234567890, 0, 0)]
    taxa = rng.sample(range(1, 1 << 32), 3000)
    big = [(2, t, rng.randrange(1 << 32), rng.randrange(0, 40), rng.randrange(2), rng.randrange(1 << 40)) for t in taxa for _ in range(rng.choice((1, 2, 2)))]
    rng.shuffle(big)
    rows += big
    rows += [(5, 9, 1, 0, 0, 1)]
    hits = hits_of(rows)
    ids = ["first", "", "a read with spaces", "x", "y", "last/1"]
    want = M.format_results(hits, ids)
    got = A.collapse(hits)
    assert len([g for g in got if g[0] == 2]) == 3000
    assert M.format_assignments(A.as_array(got, M.ASSIGN_DTYPE), ids) == want
    assert want.startswith("first:0=1234567890,4294967295=4000000000\n")
    assert A.text(got, ids) == want
    assert M.format_assignments(np.zeros(0, dtype=M.ASSIGN_DTYPE), ids) == ""


def test_formatter_on_100000_lines():
    rng = np.random.default_rng(8)
    n = 100_000
    k = rng.integers(1, 4, size=n)
    read = np.repeat(np.arange(n, dtype=np.uint64) * 2, k)          # every other read has no line
    hits = np.zeros(len(read), dtype=M.HIT_DTYPE)
    hits["read"] = read
    hits["tax_id"] = rng.integers(1, 50, size=len(read))
    hits["edit"] = rng.integers(0, 30, size=len(read))
    ids = [f"r{i}" for i in range(2 * n)]
    want = M.format_results(hits, ids)
    assert want.count("\n") == n
    assert M.format_assignments(A.as_array(A.collapse(hits), M.ASSIGN_DTYPE), ids) == want


def test_formatter_refusals():
    ids = ["a", "b", "c"]
    ok = A.as_array([(0, 1, 0), (2, 1, 0)], M.ASSIGN_DTYPE)
    assert M.format_assignments(ok, ids) == "a:1=0\nc:1=0\n"
    for bad in ([(2, 1, 0), (0, 1, 0)],            # reads out of order
                [(0, 1, 0), (1, 1, 0), (0, 2, 0)],
                [(3, 1, 0)],                       # a read >= n_reads
                [(0, 1, 0), (1 << 40, 1, 0)]):
        with pytest.raises(M.MtsvError) as e:
            M.format_assignments(A.as_array(bad, M.ASSIGN_DTYPE), ids)
        assert e.value.code == _lib.E_ARG
