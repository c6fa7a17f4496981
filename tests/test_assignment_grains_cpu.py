"""The wide grains of the assignments, the parts that need no device: the struct, the semantics restated in Python
(grain_ref.py) against the oracle's own long lines and against mtsv-collapse --mode taxid-gi on per-chunk long files, the
formatter mtsv_format_assignments_gi against mtsv_format_results(long_format = 1), its refusals."""
import os
import random
import subprocess

import numpy as np
import pytest

import grain_cases as G
import grain_ref as GR
import helpers
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLAPSE = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")


def hits_of(rows):
    """(read, tax_id, gi, edit, strand, offset) rows as a HIT_DTYPE array"""
    out = np.zeros(len(rows), dtype=M.HIT_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def oracle_lines(hits, ids):
    return "".join(O.format_line(ids[r], hits[hits["read"] == r], long_format=True) for r in sorted(set(hits["read"].tolist())))


@pytest.fixture(scope="module")
def chunks():
    first, second, seg, half, rng = G.database()
    reads = G.reads(rng, seg, half, first, n_seg=12, n_pal=6, n_bg=12)
    bases, off = helpers.reads_to_batch(reads)
    parts = [O.Index.build(e).bin_batch(bases, off, O.default_params(), threads=8)[0] for e in (first, second)]
    return parts, [f"R{i}" for i in range(len(reads))]


def test_struct_layout():
    assert M.ASSIGN_GI_DTYPE.itemsize == 24
    assert [M.ASSIGN_GI_DTYPE.fields[f][1] for f in ("read", "tax_id", "gi", "offset", "edit")] == [0, 8, 12, 16, 20]
    assert (M.GRAIN_TAXID, M.GRAIN_TAXID_GI, M.GRAIN_LONG) == (0, 1, 2)
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    assert "} mtsv_assignment_gi;" in src
    for name, v in (("MTSV_GRAIN_TAXID", 0), ("MTSV_GRAIN_TAXID_GI", 1), ("MTSV_GRAIN_LONG", 2)):
        assert f"#define {name} {v}\n" in src
    for sym in ("mtsv_batch_set_assignment_grain", "mtsv_batch_download_assignments_gi", "mtsv_format_assignments_gi"):
        assert sym in _lib.EXPORTS and sym in src


def test_restatement_on_hand_made_hits():
    B = 1 << 31
    hits = hits_of([(0, 7, 1, 3, 0, 10), (0, 7, 1, 1, 1, 10),                     # one long key twice, the smaller edit second
                    (0, 7, 1, 1, 0, 4), (0, 7, 1, 2, 1, 2),                       # the same pair: equal edits, the offset decides
                    (1, B + 5, 1, 2, 0, 1), (1, 5, 9, 0, 0, 2), (1, 5, B + 2, 4, 1, 3), (1, 5, 3, 4, 1, 3),  # bit 31 in tax_id and in gi
                    (3, 9, 9, 6, 0, 0xFFFFFFFF), (3, 9, 9, 6, 1, 0), (3, 9, 9, 6, 1, 0)])
    long_want = [(0, 7, 1, 2, 2), (0, 7, 1, 4, 1), (0, 7, 1, 10, 1),
                 (1, 5, 3, 3, 4), (1, 5, 9, 2, 0), (1, 5, B + 2, 3, 4), (1, B + 5, 1, 1, 2),
                 (3, 9, 9, 0, 6), (3, 9, 9, 0xFFFFFFFF, 6)]
    gi_want = [(0, 7, 1, 4, 1), (1, 5, 3, 3, 4), (1, 5, 9, 2, 0), (1, 5, B + 2, 3, 4), (1, B + 5, 1, 1, 2), (3, 9, 9, 0, 6)]
    assert GR.collapse_long(hits) == long_want
    assert GR.collapse_taxid_gi(hits) == gi_want
    for seed in (3, 4):
        p = np.random.default_rng(seed).permutation(len(hits))
        assert GR.collapse_long(hits[p]) == long_want             # the order of the hits does not matter
        assert GR.collapse_taxid_gi(hits[p]) == gi_want
    assert GR.collapse_long(hits[:0]) == [] and GR.collapse_taxid_gi(hits[:0]) == []
    ids = ["a", "b", "c", "d"]
    assert GR.text(gi_want, ids) == f"a:7-1-4=1\nb:5-3-3=4,5-9-2=0,5-{B + 2}-3=4,{B + 5}-1-1=2\nd:9-9-0=6\n"
    assert GR.text([], ids) == ""
    assert GR.as_tuples(GR.as_array(long_want, M.ASSIGN_GI_DTYPE)) == long_want


def test_long_restatement_against_the_oracle_lines_on_the_tricky_database():
    entries, gene, unit = helpers.tricky_db(seed=7)
    orc = O.Index.build(entries)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=12, lengths=(150,))
    bases, off = helpers.reads_to_batch(reads)
    hits, _ = orc.bin_batch(bases, off, O.default_params(), threads=8)
    ids = [f"R{i}" for i in range(len(reads))]
    want = oracle_lines(hits, ids)
    got = GR.collapse_long(hits)
    assert len(got) > 50
    assert GR.text(got, ids) == want
    assert M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids) == want
    assert M.format_results(hits, ids, long_format=True) == want


def test_long_restatement_against_the_oracle_lines_on_chunk_a(chunks):
    parts, ids = chunks
    hits = parts[0]
    c = G.census(hits)
    assert c["tax31"] and c["gi31"] and c["by_offset"] and c["winner_later"] and c["offset_decides"] and c["same_edit"], c
    want = oracle_lines(hits, ids)
    got = GR.collapse_long(hits)
    assert len(got) == len(hits) - c["same_edit"]
    assert GR.text(got, ids) == want
    assert M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids) == want


def test_taxid_gi_restatement_against_mtsv_collapse_on_the_chunk_files(chunks, tmp_path):
    parts, ids = chunks
    both = np.concatenate(parts)
    c = G.census(both)
    assert c["tax31"] and c["gi31"] and c["offset_decides"] and c["by_edit"] and c["edit_later"] and c["winner_later"] and c["group_max"] == 4, c
    files = []
    for k, p in enumerate(parts):
        f = tmp_path / f"chunk{k}.long"
        f.write_text(M.format_results(p, ids, long_format=True))
        files.append(str(f))
    out = tmp_path / "collapsed.txt"
    r = subprocess.run([COLLAPSE, "--mode", "taxid-gi", "-o", str(out), *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = GR.collapse_taxid_gi(both)
    assert len(got) < len(GR.collapse_long(both)) < len(both)
    assert sorted(GR.text(got, ids).splitlines()) == sorted(out.read_text().splitlines())
    assert sorted(M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids).splitlines()) == sorted(out.read_text().splitlines())


def test_formatter_equals_format_results_on_hand_made_hits():
    rng = random.Random(5)
    top = 4294967295
    # read 0: the largest TaxID, GI and offset the device has, ten-digit edits; read 2: 3000 long keys, most of them twice
    rows = [(0, top, top, top, 0, top), (0, top, top, 4000000000, 1, top), (0, top, top - 1, 7, 0, top), (0, 0, 0, 1234567890, 0, 0)]
    keys = [(rng.randrange(1, 1 << 32), rng.randrange(1 << 32), rng.randrange(1 << 32)) for _ in range(1000)]
    keys += [(t, g, rng.randrange(1 << 32)) for t, g, _ in keys[:500]] + [(t, rng.randrange(1 << 32), o) for t, _, o in keys[:500]]
    keys += [(7, 7, o) for o in rng.sample(range(1 << 32), 1000)]
    assert len(set(keys)) == 3000
    big = [(2, t, g, rng.randrange(0, 40), rng.randrange(2), o) for t, g, o in keys for _ in range(rng.choice((1, 2, 2)))]
    rng.shuffle(big)
    rows += big + [(5, 9, 1, 0, 0, 1)]
    hits = hits_of(rows)
    ids = ["first", "", "a read with spaces", "x", "y", "last/1"]
    want = M.format_results(hits, ids, long_format=True)
    got = GR.collapse_long(hits)
    assert len([g for g in got if g[0] == 2]) == 3000
    assert M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids) == want
    assert want.startswith(f"first:0-0-0=1234567890,{top}-{top - 1}-{top}=7,{top}-{top}-{top}=4000000000\n")
    assert GR.text(got, ids) == want
    assert M.format_assignments_gi(np.zeros(0, dtype=M.ASSIGN_GI_DTYPE), ids) == ""


def test_formatter_on_100000_lines():
    rng = np.random.default_rng(8)
    n = 100_000
    k = rng.integers(1, 4, size=n)
    read = np.repeat(np.arange(n, dtype=np.uint64) * 2, k)          # every other read has no line
    hits = np.zeros(len(read), dtype=M.HIT_DTYPE)
    hits["read"] = read
    hits["tax_id"] = rng.integers(1, 5, size=len(read))
    hits["gi"] = rng.integers(1, 3, size=len(read))
    hits["offset"] = rng.integers(0, 3, size=len(read))
    hits["edit"] = rng.integers(0, 30, size=len(read))
    ids = [f"r{i}" for i in range(2 * n)]
    want = M.format_results(hits, ids, long_format=True)
    assert want.count("\n") == n
    got = GR.collapse_long(hits)
    assert len(got) < len(hits)
    assert M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids) == want


def test_formatter_refusals():
    ids = ["a", "b", "c"]
    ok = GR.as_array([(0, 1, 2, 3, 0), (2, 1, 2, 3, 0)], M.ASSIGN_GI_DTYPE)
    assert M.format_assignments_gi(ok, ids) == "a:1-2-3=0\nc:1-2-3=0\n"
    for bad in ([(2, 1, 2, 3, 0), (0, 1, 2, 3, 0)],            # reads out of order
                [(0, 1, 2, 3, 0), (1, 1, 2, 3, 0), (0, 2, 2, 3, 0)],
                [(3, 1, 2, 3, 0)],                             # a read >= n_reads
                [(0, 1, 2, 3, 0), (1 << 40, 1, 2, 3, 0)]):
        with pytest.raises(M.MtsvError) as e:
            M.format_assignments_gi(GR.as_array(bad, M.ASSIGN_GI_DTYPE), ids)
        assert e.value.code == _lib.E_ARG
