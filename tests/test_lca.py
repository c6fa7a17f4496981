"""-m gpu tests of the per-read LCA and the clade rows (k_lca.hip, mtsv_fold_lca, mtsv-collapse --taxonomy).

Synthetic records through mtsv_fold_add_records, no index.  Expected values never come from the device: they are lca_ref's --
the LCA by intersecting ancestor chains, the clade sums by walking every read's LCA to the root -- of the same records.
Every comparison is exact, and every case is checked in five ways (check): the output fold's records, its text, its taxa
report (every row only_hit, equal to `direct`), its flags (equal to the source fold's), and the clade rows."""
import collections
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import lca_ref as R
import mtsv_tools_amd as M
import parse_cases as PC
import parse_ref as P
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "nodes_primates.dmp")
GRAINS = {"taxid": M.GRAIN_TAXID, "taxid_gi": M.GRAIN_TAXID_GI, "long": M.GRAIN_LONG}
ALL = M.SLACK_ALL
N_STAR = 5000
STAR = "1 | 1 | root\n" + "".join(f"{10 + k} | 1 | leaf\n" for k in range(N_STAR))                      # a root with 5000 children, 10 .. 5009
CHAIN = "1 | 1 | top\n" + "".join(f"{k} | {k - 1} | link\n" for k in range(2, 301))                   # 300 nodes, one under the other
HIGH = "2147483648 | 2147483648 | a\n2147483649 | 2147483648 | b\n4000000000 | 2147483648 | b\n5 | 2147483648 | c\n7 | 4000000000 | c\n4294967295 | 4000000000 | d\n"
# for the golden results: TaxIDs 2 3 5 8 9 17 31 40 64 123456 known, 77 and 4000000000 not; 400 is an implied root, 64 a root
E2E = ("1 | 1 | no rank\n100 | 1 | family\n200 | 100 | genus\n2 | 200 | species\n3 | 200 | species\n5 | 200 | species\n300 | 100 | genus\n"
       "8 | 300 | species\n9 | 300 | species\n17 | 100 | genus\n31 | 400 | species\n40 | 400 | species\n64 | 64 | no rank\n123456 | 1 | species\n")


class Tax:
    """a taxonomy twice: the restatement's and the library's"""

    def __init__(self, path):
        self.path = str(path)
        self.ref = R.Taxonomy(open(path).read())
        self.lib = M.Taxonomy(self.path)


@pytest.fixture(scope="module")
def taxa(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxonomies")
    out = {"primates": Tax(FIXTURE)}
    for name, text in (("star", STAR), ("chain", CHAIN), ("high", HIGH), ("e2e", E2E)):
        (d / f"{name}.dmp").write_text(text)
        out[name] = Tax(d / f"{name}.dmp")
    return out


def as_array(grain, recs):
    """(read, tax, edit) triples, put in key order, as the records of the grain; a wide record gets GI 7 and offset 3, or the
    (gi, offset) given"""
    recs = sorted(recs)
    if grain == M.GRAIN_TAXID:
        a = np.zeros(len(recs), dtype=M.ASSIGN_DTYPE)
        for k, (read, tax, edit) in enumerate(recs):
            a[k] = (read, tax, edit)
        return a
    a = np.zeros(len(recs), dtype=M.ASSIGN_GI_DTYPE)
    for k, r in enumerate(recs):
        a[k] = (r[0], r[1], 7, 3, r[2]) if len(r) == 3 else r
    return a


def raw(fold):
    return (fold.download() if fold.grain == M.GRAIN_TAXID else fold.download_gi()).tobytes()


def ids_of(n_reads):
    return [f"read/{k}" for k in range(n_reads)]


def check(fold, tax, recs, n_reads, slack, out=None, flags=True):
    """mtsv_fold_lca of `fold`, which holds `recs`, against the restatement, in the five ways; returns the rows"""
    want = R.per_read(tax.ref, recs, slack)
    before = (fold.count(), raw(fold))
    own = out is None
    if own:
        out = M.Fold(0, M.GRAIN_TAXID)
    rows, total, ms = fold.lca(tax.lib, slack, out=out)
    assert (fold.count(), raw(fold)) == before and ms >= 0
    # 1. the records
    got = out.download()
    assert list(zip(got["read"].tolist(), got["tax_id"].tolist(), got["edit"].tolist())) == want
    assert out.count() == len(want) and total == len(want)
    if flags:
        # 2. the text
        ids = ids_of(n_reads)
        assert out.format_text(ids)[0] == R.lca_lines(want, ids)
        # 3. the taxa report: every row only_hit, equal to direct
        direct = collections.Counter(t for _, t, _ in want)
        trows, ttotal, _ = out.taxa_report()
        assert dict(zip(trows["tax_id"].tolist(), trows["only_hit"].tolist())) == dict(direct) and ttotal == len(want)
        assert list(trows["tax_id"]) == sorted(direct)
        assert not (trows["only_best"].any() or trows["tied_best"].any() or trows["not_best"].any())
        # 4. the flags
        f_out, m_out = out.match_flags()
        f_src, m_src = fold.match_flags()
        assert len(f_out) == n_reads and np.array_equal(f_out, f_src) and m_out == m_src == len(want)
    # 5. the clade rows
    want_rows = [(t, p, code, depth, d, c) for t, p, _, code, depth, d, c in R.clade_rows(tax.ref, want)]
    assert [tuple(r) for r in rows.tolist()] == want_rows
    assert not want_rows or (rows[0]["tax_id"] == 0 and rows[0]["clade"] == total)
    # the same rows without an output fold
    rows2, total2, _ = fold.lca(tax.lib, slack)
    assert rows2.tobytes() == rows.tobytes() and total2 == total
    if own:
        out.close()
    return rows


def run(grain, tax, recs, n_reads, slacks=(0,), flags=True):
    fold = M.Fold(0, grain, n_reads=n_reads)
    fold.add_records(as_array(grain, recs))
    for s in slacks:
        check(fold, tax, recs, n_reads, s, flags=flags)
    fold.close()


def random_list(rng, pool, n_reads, longest, max_edit=4, skip=0.2):
    recs = []
    for read in range(n_reads):
        if rng.random() < skip:
            continue
        k = rng.choice((1, 1, 2, 3, 5, rng.randrange(1, longest + 1)))
        for t in sorted(rng.sample(pool, min(k, len(pool)))):
            recs.append((read, t, rng.randrange(max_edit + 1)))
    return recs


def set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("MTSV_LCA_TILE", raising=False)
    else:
        monkeypatch.setenv("MTSV_LCA_TILE", tile)


# ---- 1. tile sizes and grains ----

@pytest.mark.parametrize("tile", ["64", None], ids=["tile64", "default_tile"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_random_lists_at_both_tiles_and_all_grains(gname, tile, monkeypatch, taxa):
    set_tile(monkeypatch, tile)
    tax = taxa["primates"]
    pool = tax.ref.listed + tax.ref.implied + [0, 77, 4000000001]
    recs = random_list(random.Random(3), pool, 400, 80)
    assert len(recs) > 2000 and len({r[0] for r in recs}) > 250
    run(GRAINS[gname], tax, recs, 400, slacks=(0, 1, ALL))


@pytest.mark.parametrize("gname", ["taxid_gi", "long"])
def test_wide_grains_repeat_a_taxid(gname, monkeypatch, taxa):
    set_tile(monkeypatch, "64")
    tax = taxa["primates"]
    rng = random.Random(4)
    recs = []
    for read, t, e in random_list(rng, tax.ref.listed + [77], 120, 30):
        for gi in (1, 0x80000001)[:rng.randrange(1, 3)]:
            for off in (0, 9) if gname == "long" and rng.random() < 0.5 else (4,):
                recs.append((read, t, gi, off, (e + rng.randrange(3)) if gi > 1 else e))
    recs.sort()
    # all the records of a read of one TaxID: it is its own LCA
    recs += [(130, 9606, g, 1, 2 + g % 3) for g in range(1, 150)]
    run(GRAINS[gname], tax, recs, 131, slacks=(0, 2))


# ---- 2. where a read lies in its tile ----

def star_read(read, first, count, edit=2):
    return [(read, 10 + first + k, edit) for k in range(count)]


@pytest.mark.parametrize("first_len", [62, 63, 64, 65, 66, 128, 129])
def test_a_read_that_ends_at_a_tile_edge(first_len, monkeypatch, taxa):
    # tile 64: the first read's last record at position 61 .. 65 (and 127, 128); behind it reads that lie inside the next tile
    set_tile(monkeypatch, "64")
    recs = star_read(0, 0, first_len)
    for read in range(1, 40):
        recs += star_read(read, 7 * read, 1 + read % 4, edit=read % 3)
    recs += star_read(41, 100, 70) + star_read(42, 5, 1)
    run(M.GRAIN_TAXID, taxa["star"], recs, 43, slacks=(0, ALL))


@pytest.mark.parametrize("tile", ["64", "256", None])
def test_the_filter_waits_for_the_smallest_edit(tile, monkeypatch, taxa):
    # a read of 600 records over ten tiles of 64 whose smallest edit is its last record's: with slack 0 only that record enters,
    # so the LCA is its TaxID; a tile that filtered by its own minimum would let its records in and give the root
    set_tile(monkeypatch, tile)
    recs = star_read(0, 0, 30) + star_read(1, 0, 599, edit=5) + [(1, 10 + 599, 1)] + star_read(2, 3, 2)
    tax = taxa["star"]
    assert R.per_read(tax.ref, recs, 0)[1] == (1, 10 + 599, 1) and R.per_read(tax.ref, recs, 4)[1] == (1, 1, 1)
    run(M.GRAIN_TAXID, tax, recs, 3, slacks=(0, 3, 4))
    # ... and when it is the first record's, in an earlier tile
    recs = star_read(0, 0, 30) + [(1, 10, 1)] + star_read(1, 1, 599, edit=5) + star_read(2, 3, 2)
    run(M.GRAIN_LONG, tax, recs, 3, slacks=(0, 4))


def test_one_read_of_5000_records_and_a_scan_over_5002_nodes(taxa, monkeypatch):
    # default tile: five tiles of one read; the tree has the root's 5000 children, so the scan over `direct` crosses its tiles,
    # with reads on the first and on the last child
    set_tile(monkeypatch, None)
    recs = star_read(0, 0, N_STAR) + [(1, 10, 0)] + [(2, 10 + N_STAR - 1, 3)] + [(3, 10, 1), (3, 10 + N_STAR - 1, 1)] + [(5, 10 + N_STAR - 1, 0)]
    rows = check_once(M.GRAIN_TAXID, taxa["star"], recs, 6, 0)
    assert [tuple(r)[:1] + tuple(r)[4:] for r in rows.tolist()] == [(0, 0, 5), (1, 2, 5), (10, 1, 1), (10 + N_STAR - 1, 2, 2)]


def check_once(grain, tax, recs, n_reads, slack):
    fold = M.Fold(0, grain, n_reads=n_reads)
    fold.add_records(as_array(grain, recs))
    rows = check(fold, tax, recs, n_reads, slack)
    fold.close()
    return rows


# ---- 3. slack ----

@pytest.mark.parametrize("slack", [0, 1, 3, ALL])
def test_slack_values(slack, taxa, monkeypatch):
    set_tile(monkeypatch, "64")
    tax = taxa["primates"]
    B = 0xffffffff
    recs = [(0, 9598, 2), (0, 9606, 2), (0, 9593, 3), (0, 9583, 5),        # ties at m; one more taxon per slack
            (1, 9606, B - 1), (1, 9598, B), (1, 9583, B - 3),                # m + slack saturates
            (2, 63221, 7),                                                   # the only record enters
            (3, 9606, B), (3, 9593, B),                                      # m itself all ones
            (4, 9597, 0), (4, 756884, 1), (4, 9606, 4),
            (6, 9606, 3), (6, 9604, 3), (6, 63221, 3)]                       # an ancestor and its descendants
    want = {r: t for r, t, _ in R.per_read(tax.ref, recs, slack)}
    assert want[0] == {0: 9604, 1: 9604, 3: 0, ALL: 0}[slack] and want[2] == 63221 and want[3] == 9604 and want[6] == 9604
    assert want[1] == {0: 9583, 1: 9583, 3: 0, ALL: 0}[slack]
    assert want[4] == {0: 9597, 1: 9596, 3: 9596, ALL: 9604}[slack]
    for grain in GRAINS.values():
        check_once(grain, tax, recs, 7, slack)


# ---- 4. tree shapes ----

def test_a_chain_of_300_nodes(taxa, monkeypatch):
    set_tile(monkeypatch, "64")
    recs = [(0, 1, 0), (0, 300, 0), (1, 300, 1), (2, 299, 0), (2, 300, 0), (3, 150, 2), (3, 300, 2), (4, 1, 9)]
    recs += [(5, k, 1) for k in range(40, 301)] + [(6, 300, 0), (6, 301, 0)]         # 301: not in the taxonomy
    tax = taxa["chain"]
    assert [t for _, t, _ in R.per_read(tax.ref, recs, 0)] == [1, 300, 299, 150, 1, 40, 0]
    rows = check_once(M.GRAIN_TAXID, tax, recs, 7, 0)
    assert rows["depth"].max() == 300 and len(rows) == 301                            # the chain and the super-root


def test_taxids_with_bit_31_set(taxa):
    tax = taxa["high"]
    recs = [(0, 5, 1), (0, 2147483649, 1), (1, 7, 0), (1, 4294967295, 0), (2, 4294967295, 3), (3, 2147483649, 2), (3, 7, 2),
            (4, 2147483648, 0), (5, 4294967294, 1), (6, 4294967294, 0), (6, 4294967295, 0), (7, 5, 0)]
    assert [t for _, t, _ in R.per_read(tax.ref, recs, 0)] == [2147483648, 4000000000, 4294967295, 2147483648, 2147483648, 4294967294, 0, 5]
    for grain in GRAINS.values():
        rows = check_once(grain, tax, recs, 8, 0)
    # children ascending by TaxID as unsigned; the unknown TaxID a child of the super-root, behind the root
    assert rows["tax_id"].tolist() == [0, 2147483648, 5, 4000000000, 4294967295, 4294967294]


def test_unknown_taxids_and_implied_roots(taxa):
    tax = taxa["primates"]
    recs = [(0, 77, 1), (1, 77, 0), (1, 9606, 0), (2, 77, 2), (2, 4000000001, 2), (3, 9606, 1), (3, 9583, 1),   # 9583 is under 9573, 9606 under 1
            (4, 1, 0), (4, 9573, 0), (5, 9573, 4), (6, 1, 0), (6, 131567, 0), (7, 0, 0), (7, 9606, 0), (8, 0, 3)]
    assert [t for _, t, _ in R.per_read(tax.ref, recs, 0)] == [77, 0, 0, 0, 0, 9573, 1, 0, 0]
    for grain in GRAINS.values():
        check_once(grain, tax, recs, 9, 0)


# ---- 5. read numbers above 2^32 ----

def test_reads_numbered_above_2_to_32(taxa):
    n_reads = 2 ** 33 + 10
    recs = [(3, 9606, 1), (3, 9598, 1), (2 ** 32 - 1, 9606, 0), (2 ** 32, 9593, 0), (2 ** 32, 9606, 0), (2 ** 32 + 5, 9597, 2), (2 ** 33 + 1, 9606, 2),
            (2 ** 33 + 1, 63221, 1)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=n_reads)
    fold.add_records(as_array(M.GRAIN_TAXID, recs))
    check(fold, taxa["primates"], recs, n_reads, 0, flags=False)
    fold.close()


# ---- 6. fold states ----

def test_an_empty_fold(taxa):
    tax = taxa["primates"]
    fold = M.Fold(0, M.GRAIN_TAXID_GI, n_reads=9)
    out = M.Fold(0, M.GRAIN_TAXID, n_reads=3)
    out.add_records(as_array(M.GRAIN_TAXID, [(1, 5, 5)]))
    rows, total, _ = fold.lca(tax.lib, 0, out=out)
    assert len(rows) == 0 and total == 0 and out.count() == 0 and len(out.download()) == 0
    flags, matched = out.match_flags()
    assert len(flags) == 9 and matched == 0                                           # as after mtsv_fold_reset(out, 9)
    assert out.format_text(ids_of(9))[0] == b"" and len(out.taxa_report()[0]) == 0
    assert M.format_clade_report(rows, total, tax.lib) == R.HEADER.encode()
    fold.close()
    out.close()


def test_second_call_after_new_taxids_rebuilds_the_tree(taxa, monkeypatch, capfd):
    monkeypatch.setenv("MTSV_LCA_TIMING", "1")
    set_tile(monkeypatch, "64")
    tax = taxa["primates"]

    def rebuilt():
        return [int(x) for x in re.findall(r"\[lca timing\] .* rebuilt (\d);", capfd.readouterr().err)]

    first = [(0, 9606, 1), (0, 9598, 1), (2, 9597, 0)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=6)
    out = M.Fold(0, M.GRAIN_TAXID)
    fold.add_records(as_array(M.GRAIN_TAXID, first))
    check(fold, tax, first, 6, 0, out=out)
    assert rebuilt() == [1, 0]                                                        # (check calls twice: with and without out)
    more = [(0, 9593, 1), (3, 77, 0), (4, 9583, 2), (4, 9606, 2)]                     # a new TaxID for read 0, new reads
    fold.add_records(as_array(M.GRAIN_TAXID, more))
    both = sorted(first + more)
    check(fold, tax, both, 6, 0, out=out)                                             # the same output fold again
    assert rebuilt() == [1, 0]
    other = Tax(tax.path)                                                             # another taxonomy object: a new tree
    check(fold, other, both, 6, ALL, out=out)
    assert rebuilt() == [1, 0]
    # an output fold that holds more than it gets
    big = M.Fold(0, M.GRAIN_TAXID, n_reads=100000)
    big.add_records(as_array(M.GRAIN_TAXID, [(r, 9606, 0) for r in range(70000)]))
    check(fold, tax, both, 6, 0, out=big)
    for f in (fold, out, big):
        f.close()


def test_an_output_fold_that_must_grow(taxa):
    tax = taxa["primates"]
    n = 70000                                                                         # above the first allocation of a fold
    recs = [(r, (9606, 9598, 9593)[r % 3], r % 5) for r in range(n)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=n)
    fold.add_records(as_array(M.GRAIN_TAXID, recs))
    out = M.Fold(0, M.GRAIN_TAXID, n_reads=2)
    out.add_records(as_array(M.GRAIN_TAXID, [(1, 5, 5)]))
    rows, total, _ = fold.lca(tax.lib, 0, out=out)
    got = out.download()
    assert total == n and np.array_equal(got["read"], np.arange(n)) and got["tax_id"].tolist() == [r[1] for r in recs]
    assert got["edit"].tolist() == [r[2] for r in recs]
    by_tax = {int(r["tax_id"]): int(r["direct"]) for r in rows}
    assert (by_tax[9606], by_tax[9598], by_tax[9593]) == (23334, 23333, 23333) and int(rows[0]["clade"]) == n
    fold.close()
    out.close()


# ---- 7. refusals ----

def test_refusals_leave_both_folds_as_they_were(taxa):
    tax = taxa["primates"]
    L = M.lib()
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=5)
    fold.add_records(as_array(M.GRAIN_TAXID, [(0, 9606, 1), (3, 9598, 2)]))
    wide = M.Fold(0, M.GRAIN_LONG, n_reads=4)
    wide.add_records(as_array(M.GRAIN_LONG, [(2, 5, 5)]))
    narrow = M.Fold(0, M.GRAIN_TAXID, n_reads=4)
    narrow.add_records(as_array(M.GRAIN_TAXID, [(2, 5, 5)]))
    state = lambda: [(f.count(), raw(f), f.match_flags()[0].tobytes()) for f in (fold, wide, narrow)]  # noqa: E731
    before = state()
    ptr, n, total = C.c_void_p(), C.c_uint64(), C.c_uint64()

    def refused(f, tx, out, rows, n_rows, total_reads):
        rc = L.mtsv_fold_lca(f, tx, 0, out, rows, n_rows, total_reads, None)
        assert rc == _lib.E_ARG, L.mtsv_last_error()
        assert state() == before and ptr.value is None

    refused(fold.h, tax.lib.h, fold.h, None, None, None)                              # out == f
    refused(fold.h, tax.lib.h, wide.h, None, None, None)                              # out of a wide grain
    refused(wide.h, tax.lib.h, wide.h, None, None, None)
    refused(None, tax.lib.h, narrow.h, None, None, None)                              # a null f
    refused(fold.h, None, narrow.h, None, None, None)                                 # a null tx
    refused(fold.h, tax.lib.h, narrow.h, C.byref(ptr), None, C.byref(total))          # rows without n_rows
    refused(fold.h, tax.lib.h, narrow.h, C.byref(ptr), C.byref(n), None)              # rows without total_reads
    if M.device_count() > 1:
        far = M.Fold(1, M.GRAIN_TAXID, n_reads=4)
        refused(fold.h, tax.lib.h, far.h, None, None, None)                           # another device
        far.close()
    # and the call they refused works
    check(fold, tax, [(0, 9606, 1), (3, 9598, 2)], 5, 0, out=narrow)
    for f in (fold, wide, narrow):
        f.close()


# ---- 8. round trip ----

def test_the_text_of_the_output_fold_parses_back_to_its_records(taxa, monkeypatch):
    set_tile(monkeypatch, "64")
    tax = taxa["primates"]
    recs = random_list(random.Random(8), tax.ref.listed + tax.ref.implied + [77, 4000000001], 300, 6)
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=300)
    fold.add_records(as_array(M.GRAIN_TAXID, recs))
    out = M.Fold(0, M.GRAIN_TAXID)
    fold.lca(tax.lib, ALL, out=out)
    text = out.format_text(ids_of(300))[0].decode()
    assert re.search(r":0=\d+\n", text)                                               # reads whose taxa meet in the super-root
    reads = sorted({r[0] for r in recs})
    lines = [(read, row.rsplit(":", 1)[1]) for read, row in zip(reads, text.splitlines())]
    back = M.Fold(0, M.GRAIN_TAXID, n_reads=300)
    assert back.add_text(*P.arrays(lines))[:2] == (len(reads), len(reads))
    assert raw(back) == raw(out) and out.count() == len(reads)
    for f in (fold, out, back):
        f.close()


# ---- 9. the command line ----

def lca_tool(tmp_path, texts, *extra, env=None, tag="lca"):
    lines, clades = tmp_path / f"{tag}.lca", tmp_path / f"{tag}.clades"
    r, out, rep = PC.run_tool(tmp_path, texts, "--on-gpu", "--lca-output", str(lines), "--clade-report", str(clades), *extra, env=env, tag=tag)
    return r, out, rep, (lines.read_bytes() if lines.exists() else None), (clades.read_bytes() if clades.exists() else None)


@pytest.mark.parametrize("case", ["default/taxid/0", "long/taxid/1", "long/taxid-gi/all/pieces", "long/taxid-gi/0"])
def test_cli_golden_results_cut_into_three_files(case, tmp_path, taxa):
    name, mode, slack = case.split("/")[:3]
    tax = taxa["e2e"]
    texts = PC.golden_cut("e2e_default.results" if name == "default" else "e2e_default_long.results")
    env = {"MTSV_COLLAPSE_PIECE_BYTES": "256"} if case.endswith("pieces") else None
    plain, plain_out, plain_rep = PC.run_tool(tmp_path, texts, "--mode", mode, "--on-gpu", env=env, tag="plain")
    assert plain.returncode == 0, plain.stderr
    r, out, rep, lines, clades = lca_tool(tmp_path, texts, "--mode", mode, "--taxonomy", tax.path, "--lca-slack", slack, env=env)
    assert r.returncode == 0, r.stderr
    assert out == plain_out and rep == plain_rep and len(out) > 0 and len(rep) > 0   # -o and --report: what they are without
    ids, recs = P.collapse_files(P.TAXID if mode == "taxid" else P.TAXID_GI, texts)
    want = R.per_read(tax.ref, recs, ALL if slack == "all" else int(slack))
    assert len(want) == len(out.splitlines()) > 100
    assert lines == R.lca_lines(want, ids)
    assert [l.split(b":")[0] for l in lines.splitlines()] == [l.rsplit(b":", 1)[0] for l in out.splitlines()]  # the order of -o's lines
    assert clades == R.report_text(R.clade_rows(tax.ref, want), len(want))
    assert len({t for _, t, _ in want}) > 5 and any(t == 0 for _, t, _ in want) and any(t in (100, 200, 300) for _, t, _ in want)
    # only one of the two outputs
    only = tmp_path / "only.clades"
    r2, _, _ = PC.run_tool(tmp_path, texts, "--mode", mode, "--on-gpu", "--taxonomy", tax.path, "--lca-slack", slack, "--clade-report", str(only), env=env,
                           tag="one")
    assert r2.returncode == 0 and only.read_bytes() == clades and not (tmp_path / "one.lca").exists()


def test_cli_usage_errors(tmp_path, taxa):
    tax = taxa["e2e"]
    texts = ["a:2=1,3=1\n"]

    def usage(*args):
        r, out, _ = PC.run_tool(tmp_path, texts, *args, tag="usage")
        assert r.returncode == 1 and out is None and r.stderr.startswith("error: "), (args, r.stderr)
        assert not list(tmp_path.glob("*.lca")) and not list(tmp_path.glob("*.clades"))
        return r.stderr

    lines, clades = str(tmp_path / "u.lca"), str(tmp_path / "u.clades")
    assert "'--taxonomy <nodes.dmp>' requires '--on-gpu'" in usage("--taxonomy", tax.path, "--lca-output", lines)
    assert "requires '--lca-output <PATH>' or '--clade-report <TSV>'" in usage("--on-gpu", "--taxonomy", tax.path)
    assert "'--lca-output <PATH>' requires '--taxonomy <nodes.dmp>'" in usage("--on-gpu", "--lca-output", lines)
    assert "'--clade-report <TSV>' requires '--taxonomy <nodes.dmp>'" in usage("--on-gpu", "--clade-report", clades)
    assert "'--lca-slack <N|all>' requires '--taxonomy <nodes.dmp>'" in usage("--on-gpu", "--lca-slack", "2")
    assert "Invalid value for '--lca-slack <N|all>': some" in usage("--on-gpu", "--taxonomy", tax.path, "--lca-output", lines, "--lca-slack", "some")


@pytest.mark.parametrize("case", ["key_order", "no_offset", "taxonomy"])
def test_cli_refused_input_with_a_taxonomy_ends_non_zero(case, tmp_path, taxa):
    tax = taxa["e2e"]
    texts = {"key_order": PC.KEY_ORDER, "no_offset": PC.NO_OFFSET, "taxonomy": PC.LAYERS}[case]
    path = tax.path
    if case == "taxonomy":                                                            # a taxonomy that does not load
        path = str(tmp_path / "bad.dmp")
        open(path, "w").write("2 | 1 | a\n2 | 1 | a\n")
    r, out, rep, lines, clades = lca_tool(tmp_path, texts, "--mode", "taxid-gi", "--taxonomy", path)
    assert r.returncode not in (0, 1) and lines is None and clades is None, r.stderr
    assert ("line 2:" in r.stderr) if case == "taxonomy" else ("--on-gpu:" in r.stderr and "--taxonomy needs the device path" in r.stderr)
    if case != "taxonomy":                                                            # without --taxonomy the host path takes the same input
        h, h_out, _ = PC.run_tool(tmp_path, texts, "--mode", "taxid-gi", "--on-gpu", tag="fallback")
        assert h.returncode == 0 and len(h_out) > 0
