"""-m gpu: the tiled passes (k_text, k_fold, k_parse, k_lca, k_pair, k_abund) at every tile size they accept, on the cases of
tile_cases.py that are built onto their structural edges, the upper levels of the text scan at small tiles, and the tiles of
the record kernels (k_lca.hip; k_tile.hpp) that hold no head or nothing but heads.  (The pack's scan carry:
test_device_pack.py, next to the indexes it needs.)

Expected values never come from the device or the library under test: they are the restatements' -- text_cases.text, fold_ref,
parse_ref, lca_ref, pair_ref, abund_ref -- of the same lists (test_tile_ladders_cpu.py shows that the lists hold what they claim).  Every
comparison is exact.  The tile of every run, and in part 1 the number of tiles, is asserted from the trace lines, so that a
change of a default cannot turn these into tests of one level unnoticed.  (The trace line of the abundance does not name its
tile: there the switch is set and nothing more can be asserted.  So for the abundance alone that purpose does not hold: were
MTSV_ABUND_TILE ever ignored, its five ladder levels and its tile-64 cases would all run at the default tile of 1024 and pass
unnoticed, until the tile is added to that trace line.)"""
import random
import re

import pytest

import fold_ref as F
import mtsv_tools_amd as M
import pair_cases as PC
import parse_ref as P
import text_cases as TC
import tile_cases as K
from mtsv_tools_amd import _lib
from test_abundance import as_array as abund_array
from test_abundance import check as abund_check
from test_fold import as_array, check_fold
from test_lca import ALL, Tax, check
from test_lca import as_array as lca_array
from test_pair import DT, MODES
from test_pair import check as pair_check
from test_parse_text import add, n_tokens, refused

pytestmark = pytest.mark.gpu

GRAINS = TC.GRAINS
LCA_LINE = r"\[lca\] \d+ records of \d+ reads over \d+ nodes \(\d+ TaxIDs, depth \d+\) in \d+ tiles of (\d+),"
PAIR_LINE = r"\[pair\] mode \d+, \d+ records of \d+ pairs in \d+ runs, \d+ on the work list \(lane tier up to \d+\), tiles of (\d+) "
TEXT_LINE = r"\[text\] (\d+) records -> (\d+) bytes in (\d+) tiles of (\d+) "
SCAN_CHUNK = 2048          # tiles per workgroup of k_text_scan_sums / _apply; k_text_scan_top takes `per` of those per lane
SCAN_LANES = 256


def traced_fold(monkeypatch, switch, tile, grain):
    """a fold created with the tile switch set, and tracing on"""
    monkeypatch.setenv(switch, str(tile))
    monkeypatch.setenv("MTSV_TRACE", "1")
    return M.Fold(0, grain)


# ---- 1. the upper levels of the text scan, at tiles of two records ----

@pytest.mark.parametrize("gname", ["taxid", "long"])
def test_text_scan_second_workgroup(gname, monkeypatch, capfd):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_TEXT_TILE", 2, grain)
    rng = random.Random(40 + grain)
    sizes = (4096, 4097, 4098, 9001)
    for n in sizes:
        c = TC.spread(grain, rng, n, max_id=70)
        assert len(c.records) == n and max(len(s) for s in c.ids) > 64
        fold.reset(len(c.ids))
        fold.add_records(as_array(grain, c.records))
        assert fold.format_text(c.table)[0] == TC.expected(grain, c), n
    fold.close()
    seen = [tuple(map(int, m)) for m in re.findall(TEXT_LINE, capfd.readouterr().err)]
    assert [(n, tiles, tile) for n, _, tiles, tile in seen] == [(n, (n + 1) // 2, 2) for n in sizes]
    assert [-(-tiles // SCAN_CHUNK) for _, _, tiles, _ in seen] == [1, 2, 2, 3]     # workgroups of the scan: sums[blockIdx.x > 0] is read


def test_text_scan_top_takes_two_sums_per_lane(monkeypatch, capfd):
    n = 1_048_578
    rec, table, ids = K.big_text(n)
    want = K.big_text_expected(rec, ids)
    fold = traced_fold(monkeypatch, "MTSV_TEXT_TILE", 2, F.TAXID)
    fold.reset(len(ids))
    fold.add_records(rec)
    got = fold.format_text(table)[0]
    fold.close()
    if got != want:                                                               # (no megabytes in the report)
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        lo = max(at - 20, 0)
        raise AssertionError(f"{len(got)} bytes for {len(want)}; first difference at byte {at}: {got[lo:at + 20]!r} for {want[lo:at + 20]!r}")
    (records, _, tiles, tile), = [tuple(map(int, m)) for m in re.findall(TEXT_LINE, capfd.readouterr().err)]
    assert (records, tiles, tile) == (n, n // 2, 2)
    blocks = -(-tiles // SCAN_CHUNK)
    assert blocks == 257 and -(-blocks // SCAN_LANES) == 2                           # per = 2 in k_text_scan_top


# ---- 2. the tile ladders ----

@pytest.mark.parametrize("T", K.TEXT_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_text_ladder(gname, T, monkeypatch, capfd):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_TEXT_TILE", T, grain)
    for name, c in K.text_cases(grain, T).items():
        fold.reset(len(c.ids))
        fold.add_records(as_array(grain, c.records))
        assert fold.format_text(c.table)[0] == TC.expected(grain, c), name
        fold.add_records(as_array(grain, c.second))
        assert fold.format_text(c.table)[0] == TC.text(grain, F.fold(grain, c.records, c.second), c.ids), name
    fold.close()
    assert {m[3] for m in re.findall(TEXT_LINE, capfd.readouterr().err)} == {str(T)}


@pytest.mark.parametrize("T", K.FOLD_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_fold_ladder(gname, T, monkeypatch, capfd):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_FOLD_TILE", T, grain)
    for name, (a, b) in K.fold_cases(grain, T).items():
        n_reads = max(r[0] for r in a + b) + 3
        want = F.fold(grain, a, b)
        for first, second in ((a, b), (b, a)):
            fold.reset(n_reads)
            fold.add_records(as_array(grain, first))
            check_fold(fold, first, n_reads)
            fold.add_records(as_array(grain, second))
            check_fold(fold, want, n_reads)
    fold.close()
    tiles = set(re.findall(r"\[fold\] \d+ \+ \d+ records -> \d+ in \d+ tiles of (\d+)", capfd.readouterr().err))
    assert tiles == {str(T)}


@pytest.mark.parametrize("T", K.PARSE_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_parse_ladder(gname, T, monkeypatch, capfd):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_PARSE_TILE", T, grain)
    sizes = []
    for name, lines in K.parse_texts(T).items():
        if grain not in K.parse_grains(name):
            continue
        n_reads = lines[-1][0] + 1
        want = P.records(grain, lines, n_reads)
        fold.reset(n_reads)
        tok, rec, _ = add(fold, lines)
        assert (tok, rec) == (n_tokens(lines), len(want)), name
        check_fold(fold, want, n_reads)
        sizes.append(sum(len(h) for _, h in lines))
    # a token outside the grammar that starts in the last bytes of a tile: refused, its line named, the fold as it was
    lines, bad = K.parse_refused(T)
    n_reads = lines[-1][0] + 1
    have = [TC.rec(grain, 1, 5, 6, 7, 8), TC.rec(grain, 4, 5, 6, 7, 2)]
    fold.reset(n_reads)
    fold.add_records(as_array(grain, have))
    refused(fold, lines, _lib.E_FORMAT, bad)
    check_fold(fold, have, n_reads)
    fold.close()
    seen = re.findall(r"\[parse\] (\d+) bytes in \d+ lines -> \d+ tokens -> \d+ records in (\d+) tiles of (\d+) bytes", capfd.readouterr().err)
    assert [tuple(map(int, m)) for m in seen] == [(n, -(-n // T), T) for n in sizes] and min(-(-n // T) for n in sizes) >= 3


@pytest.fixture(scope="module")
def outlier(tmp_path_factory):
    path = tmp_path_factory.mktemp("outlier") / "outlier.dmp"
    path.write_text(K.OUTLIER)
    return Tax(path)


LCA_LADDER = [("taxid", T) for T in K.LCA_TILES] + [("long", 64), ("long", 1024)]


@pytest.mark.parametrize("gname,T", LCA_LADDER)
def test_lca_ladder(gname, T, monkeypatch, capfd, outlier):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_LCA_TILE", T, grain)
    out = M.Fold(0, M.GRAIN_TAXID)
    for name, (recs, n_reads) in K.lca_cases(T).items():
        fold.reset(n_reads)
        fold.add_records(lca_array(grain, recs))
        for slack in (0, ALL):
            check(fold, outlier, recs, n_reads, slack, out=out)
    fold.close()
    out.close()
    assert set(re.findall(LCA_LINE, capfd.readouterr().err)) == {str(T)}


# pairs: BOTH and EITHER at the TAXID grain, where every record is a run of its own and the reads' heads stand at the edges;
# PROPER at the LONG grain, where the runs' heads do
@pytest.mark.parametrize("T", K.PAIR_TILES)
@pytest.mark.parametrize("mode,gname", [("both", "taxid"), ("either", "taxid"), ("proper", "long")])
def test_pair_ladder(mode, gname, T, monkeypatch, capfd):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_PAIR_TILE", T, grain)
    out = M.Fold(0, M.GRAIN_TAXID)
    for name, (wide, n_reads) in K.run_cases(T).items():
        if name.startswith("reads") != (gname == "taxid"):
            continue
        recs = K.narrow(wide) if gname == "taxid" else wide
        fold.reset(n_reads)
        fold.add_records(PC.as_array(grain, recs, DT))
        pair_check(fold, recs, n_reads, MODES[mode], 50, 5, out=out)
    fold.close()
    out.close()
    assert set(re.findall(PAIR_LINE, capfd.readouterr().err)) == {str(T)}


# abundance: the reads' heads at the edges at every grain, the runs' heads at the two wide ones
@pytest.mark.parametrize("T", K.ABUND_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_abundance_ladder(gname, T, monkeypatch):
    grain = GRAINS[gname]
    fold = traced_fold(monkeypatch, "MTSV_ABUND_TILE", T, grain)
    out = M.Fold(0, M.GRAIN_TAXID)
    for name, (wide, n_reads) in K.run_cases(T, "gi").items():
        if gname == "taxid" and not name.startswith("reads"):
            continue
        recs = K.narrow(wide) if gname == "taxid" else wide
        fold.reset(n_reads)
        fold.add_records(abund_array(grain, recs))
        abund_check(fold, recs, n_reads, slack=1, max_iters=2, out=out)
    fold.close()
    out.close()


# ---- 3. tiles of the record kernels without a head, and of nothing but heads ----

EDGE_CASES = [(f"headless_{w}", K.HEADLESS_T) for w in K.HEADLESS_AT] + [("full", 64), ("full", 1024)]
EDGE_IDS = [f"{name}-{T}" for name, T in EDGE_CASES]


def edge_list(name, T, kernel):
    """(records, n_reads) of an edge case for 'lca', 'pair', 'read' (the abundance at the TAXID grain, after narrow()) or 'abund'"""
    if name == "full":
        return K.full_tile_reads(T) if kernel == "lca" else K.full_tile_runs(T, "offset" if kernel == "pair" else "gi", one_run=kernel != "read")
    at = K.HEADLESS_AT[name[len("headless_"):]]
    return K.headless_reads(at) if kernel == "lca" else K.headless_runs(at, kernel)


@pytest.mark.parametrize("name,T", EDGE_CASES, ids=EDGE_IDS)
def test_lca_tiles_without_a_head_and_of_heads_alone(name, T, monkeypatch, capfd, outlier):
    recs, n_reads = edge_list(name, T, "lca")
    fold = traced_fold(monkeypatch, "MTSV_LCA_TILE", T, M.GRAIN_TAXID)
    fold.reset(n_reads)
    fold.add_records(lca_array(M.GRAIN_TAXID, recs))
    for slack in (0, ALL):
        check(fold, outlier, recs, n_reads, slack)
    fold.close()
    assert set(re.findall(LCA_LINE, capfd.readouterr().err)) == {str(T)}


@pytest.mark.parametrize("name,T", EDGE_CASES, ids=EDGE_IDS)
@pytest.mark.parametrize("mode", list(MODES))
def test_pair_tiles_without_a_head_and_of_heads_alone(mode, name, T, monkeypatch, capfd):
    recs, n_reads = edge_list(name, T, "pair")
    fold = traced_fold(monkeypatch, "MTSV_PAIR_TILE", T, M.GRAIN_LONG)
    fold.reset(n_reads)
    fold.add_records(PC.as_array(M.GRAIN_LONG, recs, DT))
    want = pair_check(fold, recs, n_reads, MODES[mode], 480, 5)
    fold.close()
    assert any(t == 5 for _, t, _ in want)                                           # the segment's pair is joined
    assert set(re.findall(PAIR_LINE, capfd.readouterr().err)) == {str(T)}


@pytest.mark.parametrize("name,T", EDGE_CASES, ids=EDGE_IDS)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_abundance_tiles_without_a_head_and_of_heads_alone(gname, name, T, monkeypatch):
    recs, n_reads = edge_list(name, T, "read" if gname == "taxid" else "abund")
    if gname == "taxid":
        recs = K.narrow(recs)
    fold = traced_fold(monkeypatch, "MTSV_ABUND_TILE", T, GRAINS[gname])
    fold.reset(n_reads)
    fold.add_records(abund_array(GRAINS[gname], recs))
    for slack in (1, ALL):
        abund_check(fold, recs, n_reads, slack=slack, max_iters=2)
    fold.close()
