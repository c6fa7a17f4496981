"""CPU tests of the taxonomy object and the clade report text (host-only calls of the ABI) against the plain-Python
restatement in lca_ref.py, and of the restatement's two LCA forms against each other."""
import os
import random

import numpy as np
import pytest

import lca_ref as R
import mtsv_tools_amd as M
from mtsv_tools_amd import CLADE_STATS_DTYPE, Taxonomy, _lib, format_clade_report  # noqa: F401  (what this module is about)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "nodes_primates.dmp")


@pytest.fixture(scope="module")
def ref():
    return R.Taxonomy(open(FIXTURE).read())


@pytest.fixture(scope="module")
def tx():
    return M.Taxonomy(FIXTURE)


def test_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    for name in ("mtsv_taxonomy_load", "mtsv_taxonomy_free", "mtsv_taxonomy_info", "mtsv_taxonomy_parent", "mtsv_taxonomy_rank_name",
                 "mtsv_fold_lca", "mtsv_format_clade_report"):
        assert name in src and name in _lib.EXPORTS and hasattr(M.lib(), name)
    assert M.CLADE_STATS_DTYPE.itemsize == 32
    for name in ("Taxonomy", "format_clade_report", "CLADE_STATS_DTYPE"):
        assert hasattr(M, name)
    assert hasattr(M.Fold, "lca")


def test_fixture_facts(ref):
    # what the issue states about the fixture, on the restatement
    assert len(ref.listed) == 82 and ref.implied == [1, 9573]
    assert len(ref.parent) + 1 == 85 and ref.max_depth == 27
    assert ref.lca([9606, 9598]) == 9604
    assert ref.lca([63221, 741158]) == 9606
    assert ref.lca([9597, 756884]) == 9596
    assert ref.lca([9593, 9606]) == 9604
    assert ref.lca([9583, 9606]) == 0


def test_fixture_through_the_abi(ref, tx):
    assert tx.info() == {"n_nodes": 82, "n_implied_roots": 2, "n_ranks": len(ref.rank_names), "max_depth": 27}
    for t in ref.listed + ref.implied + [0, 5, 9572, 0xffffffff]:
        parent, rank = tx.parent(t)
        assert parent == ref.parent_of(t), t
        assert rank == ref.rank_code(t), t
        assert tx.rank_name(rank) == ref.rank_name(t), t
    assert [tx.rank_name(k).encode() for k in range(len(ref.rank_names))] == ref.rank_names
    assert tx.rank_name(M.RANK_UNKNOWN) == "-" and tx.rank_name(len(ref.rank_names)) == "-"

    def lca_abi(taxa):  # chains through mtsv_taxonomy_parent, intersected
        chains = []
        for t in taxa:
            c = [t]
            while c[-1]:
                c.append(tx.parent(c[-1])[0])
            chains.append(c)
        common = set(chains[0]).intersection(*chains[1:])
        return next(a for a in chains[0] if a in common)

    for taxa, want in (([9606, 9598], 9604), ([63221, 741158], 9606), ([9597, 756884], 9596), ([9593, 9606], 9604), ([9583, 9606], 0)):
        assert lca_abi(taxa) == want


def test_ncbi_format_loads_to_the_same_tree(ref, tmp_path):
    lines = []
    for k, line in enumerate(open(FIXTURE).read().split("\n")):
        if not line.strip():
            continue
        t, p, rank = [f.strip() for f in line.split("|")]
        lines.append(f"{t}\t|\t{p}\t|\t{rank}\t|\tXX\t|\t{k % 9}\t|\t\t|")
    text = "\n\n".join(lines) + "\n"  # (with empty lines between)
    path = tmp_path / "ncbi.dmp"
    path.write_text(text)
    other = R.Taxonomy(text)
    assert other.parent == ref.parent and other.rank == ref.rank
    tx = M.Taxonomy(str(path))
    assert tx.info() == {"n_nodes": 82, "n_implied_roots": 2, "n_ranks": len(ref.rank_names), "max_depth": 27}
    for t in ref.listed + ref.implied:
        assert tx.parent(t) == (ref.parent_of(t), ref.rank_code(t))
    # CR LF line ends load too
    path.write_text(text.replace("\n", "\r\n"))
    assert M.Taxonomy(str(path)).parent(9606) == (ref.parent_of(9606), ref.rank_code(9606))


MALFORMED = {
    "two_fields": ("2 | 1 | a\n3 | 2\n", 2),
    "one_field": ("2 | 1 | a\n\n7\n", 3),
    "not_digits": ("2 | 1 | a\n3x | 2 | a\n", 2),
    "negative": ("2 | 1 | a\n3 | -2 | a\n", 2),
    "empty_id": ("2 | 1 | a\n | 2 | a\n", 2),
    "eleven_digits": ("12345678901 | 1 | a\n", 1),
    "above_u32": ("2 | 1 | a\n4 | 4294967296 | a\n", 2),
    "taxid_zero": ("2 | 1 | a\n0 | 2 | a\n", 2),
    "parent_zero": ("2 | 0 | a\n", 1),
    "listed_twice": ("2 | 1 | a\n3 | 2 | a\n4 | 2 | b\n3 | 1 | a\n", 4),
    "cycle_of_two": ("2 | 1 | a\n5 | 6 | a\n6 | 5 | a\n", 2),
    "tail_into_cycle": ("4 | 7 | a\n7 | 8 | a\n8 | 9 | a\n9 | 7 | a\n", 2),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_files_are_refused(name, tmp_path):
    text, line = MALFORMED[name]
    with pytest.raises(R.Format) as e:
        R.Taxonomy(text)
    assert e.value.line == line
    path = tmp_path / (name + ".dmp")
    path.write_text(text)
    with pytest.raises(M.MtsvError) as e:
        M.Taxonomy(str(path))
    assert e.value.code == _lib.E_FORMAT
    assert f"line {line}:" in str(e.value)


def test_largest_id_and_self_parent_roots_load(tmp_path):
    path = tmp_path / "ok.dmp"
    path.write_text("4294967295 | 4294967295 | top\n7 | 4294967295 | low\n9 | 9 | top\n")
    tx = M.Taxonomy(str(path))
    assert tx.info() == {"n_nodes": 3, "n_implied_roots": 0, "n_ranks": 2, "max_depth": 2}
    assert tx.parent(4294967295) == (0, 1) and tx.parent(7) == (4294967295, 0) and tx.parent(9) == (0, 1)


def test_unreadable_file_is_an_io_error(tmp_path):
    with pytest.raises(M.MtsvError) as e:
        M.Taxonomy(str(tmp_path / "absent.dmp"))
    assert e.value.code == _lib.E_IO
    with pytest.raises(M.MtsvError) as e:
        M.MGIndex.load(str(tmp_path / "absent.idx"))  # the code the index loader uses
    assert e.value.code == _lib.E_IO


def rows_array(rows):
    a = np.zeros(len(rows), dtype=M.CLADE_STATS_DTYPE)
    for k, (t, p, _, code, depth, direct, clade) in enumerate(rows):
        a[k] = (t, p, code, depth, direct, clade)
    return a


def test_clade_report_text(ref, tx):
    rng = random.Random(5)
    pool = ref.listed + ref.implied + [0, 77, 4000000000]
    lcas = [(r, rng.choice(pool), rng.randrange(9)) for r in range(997)]
    rows = R.clade_rows(ref, lcas)
    assert rows[0][0] == 0 and rows[0][6] == 997 and sum(r[5] for r in rows) == 997
    want = R.report_text(rows, 997)
    assert M.format_clade_report(rows_array(rows), 997, tx) == want
    assert want.startswith(R.HEADER.encode()) and want.count(b"\n") == len(rows) + 1
    # total_reads = 0: percentages of max(total_reads, 1); no rows: the header alone
    assert M.format_clade_report(rows_array(rows), 0, tx) == R.report_text(rows, 0)
    assert M.format_clade_report(rows_array([]), 0, tx) == R.HEADER.encode()
    # without a taxonomy every rank is "-"
    bare = [(t, p, "-", code, d, a, b) for t, p, _, code, d, a, b in rows]
    assert M.format_clade_report(rows_array(rows), 997) == R.report_text(bare, 997)
    # as mtsv_format_taxa_report computes its own: the same figure from the same counts
    taxa = np.zeros(1, dtype=M.TAXON_STATS_DTYPE)
    taxa[0] = (9606, 333, 0, 0, 0)
    pct = M.format_taxa_report(taxa, 997).split(b"\n")[1].split(b"\t")[2]
    one = rows_array([(9606, 9605, "species", ref.rank_code(9606), 27, 333, 333)])
    assert M.format_clade_report(one, 997, tx).split(b"\n")[1].split(b"\t")[5] == pct


def test_the_two_lca_forms_agree(ref):
    rng = random.Random(11)
    pool = ref.listed + ref.implied + [0, 77, 4000000000]
    for _ in range(3000):
        taxa = [rng.choice(pool) for _ in range(rng.randrange(1, 6))]
        assert ref.lca(taxa) == ref.lca_by_intervals(taxa), taxa
