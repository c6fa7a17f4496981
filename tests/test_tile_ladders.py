"""-m gpu: the tiled passes (k_text, k_fold, k_parse, k_lca) at every tile size they accept, on the cases of tile_cases.py that
are built onto their structural edges, and the upper levels of the text scan at small tiles.  (The pack's scan carry:
test_device_pack.py, next to the indexes it needs.)

Expected values never come from the device or the library under test: they are the restatements' -- text_cases.text, fold_ref,
parse_ref, lca_ref -- of the same lists (test_tile_ladders_cpu.py shows that the lists hold what they claim).  Every
comparison is exact.  The tile of every run, and in part 1 the number of tiles, is asserted from the trace lines, so that a
change of a default cannot turn these into tests of one level unnoticed."""
import random
import re

import pytest

import fold_ref as F
import mtsv_tools_amd as M
import parse_ref as P
import text_cases as TC
import tile_cases as K
from mtsv_tools_amd import _lib
from test_fold import as_array, check_fold
from test_lca import ALL, Tax, check
from test_lca import as_array as lca_array
from test_parse_text import add, n_tokens, refused

pytestmark = pytest.mark.gpu

GRAINS = TC.GRAINS
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
    tiles = set(re.findall(r"\[lca\] \d+ records of \d+ reads over \d+ nodes \(\d+ TaxIDs, depth \d+\) in \d+ tiles of (\d+),", capfd.readouterr().err))
    assert tiles == {str(T)}
