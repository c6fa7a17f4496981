"""-m gpu tests of the abundance step (k_abund.hip, mtsv_fold_abundance, mtsv-collapse --abundance).

Synthetic records through mtsv_fold_add_records, no index.  Expected values never come from the device: they are abund_ref's,
the definition restated with Python's int and float, of the same records.  Every comparison is for equality -- the rows, every
field of the info (the number of iterations and the last L1 included), the output fold's records, its text and its taxa report
(every row only_hit, equal to `assigned`) -- and the source fold must be byte-identical before and after (check)."""
import collections
import ctypes as C
import math
import random

import numpy as np
import pytest

import abund_ref as A
import mtsv_tools_amd as M
import parse_cases as PC
import parse_ref as P
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

GRAINS = {"taxid": M.GRAIN_TAXID, "taxid_gi": M.GRAIN_TAXID_GI, "long": M.GRAIN_LONG}
ALL = M.SLACK_ALL
KNOBS = ("MTSV_ABUND_TILE", "MTSV_ABUND_LANE_MAX", "MTSV_ABUND_DENSE_MAX", "MTSV_ABUND_START_MASS", "MTSV_ALLOC_REFUSE")
W_HALF = A.weights(0.5, 64)
W_QUARTER = A.weights(0.25, 64)
TOL_DEFAULT = int(math.floor(0.01 * 4294967296.0))


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def as_array(grain, recs):
    """(read, tax, edit) triples, put in key order, as the records of the grain; a wide record gets GI 7 and offset 3, or the
    (gi, offset) given"""
    recs = sorted(recs)
    if grain == M.GRAIN_TAXID:
        return np.array([tuple(r) for r in recs], dtype=M.ASSIGN_DTYPE) if recs else np.zeros(0, dtype=M.ASSIGN_DTYPE)
    wide = [(r[0], r[1], 7, 3, r[2]) if len(r) == 3 else tuple(r) for r in recs]
    return np.array(wide, dtype=M.ASSIGN_GI_DTYPE) if wide else np.zeros(0, dtype=M.ASSIGN_GI_DTYPE)


def raw(fold):
    return (fold.download() if fold.grain == M.GRAIN_TAXID else fold.download_gi()).tobytes()


def ids_of(n_reads):
    return [f"read/{k}" for k in range(n_reads)]


def check(fold, recs, n_reads, w=W_HALF, slack=ALL, max_iters=5, tol=0, out=None, start=A.ONE, text=True):
    """mtsv_fold_abundance of `fold`, which holds `recs`, against the restatement; returns (rows, info, the restatement's result)"""
    want = A.run(recs, w, slack=slack, max_iters=max_iters, tol=tol, start=start)
    before = (fold.count(), raw(fold))
    own = out is None
    if own:
        out = M.Fold(0, M.GRAIN_TAXID)
    rows, info, ms = fold.abundance(w, slack=slack, max_iters=max_iters, tol=tol, out=out)
    assert (fold.count(), raw(fold)) == before and ms >= 0
    # the rows and the info
    assert [tuple(r) for r in rows.tolist()] == want["rows"]
    assert info == want["info"]
    # the output fold: records, text, taxa report
    got = out.download()
    assert list(zip(got["read"].tolist(), got["tax_id"].tolist(), got["edit"].tolist())) == want["assigned"]
    assert out.count() == len(want["assigned"]) == info["reads"]
    per_tax = collections.Counter(t for _, t, _ in want["assigned"])
    trows, ttotal, _ = out.taxa_report()
    assert dict(zip(trows["tax_id"].tolist(), trows["only_hit"].tolist())) == dict(per_tax) and ttotal == len(want["assigned"])
    assert list(trows["tax_id"]) == sorted(per_tax)
    assert not (trows["only_best"].any() or trows["tied_best"].any() or trows["not_best"].any())
    assert {t: n for t, _, _, _, n in want["rows"] if n} == dict(per_tax)
    if text:
        ids = ids_of(n_reads)
        assert out.format_text(ids)[0] == A.lines(want["assigned"], ids)
    # the same rows without an output fold, and nothing at all asked for
    rows2, info2, _ = fold.abundance(w, slack=slack, max_iters=max_iters, tol=tol)
    assert rows2.tolist() == rows.tolist() and info2 == info                    # (the rows have four bytes of padding: no bytes compared)
    assert fold.abundance(w, slack=slack, max_iters=max_iters, tol=tol, rows=False)[0] is None
    if own:
        out.close()
    return rows, info, want


def run(grain, recs, n_reads, **kw):
    fold = M.Fold(0, grain, n_reads=n_reads)
    fold.add_records(as_array(grain, recs))
    try:
        return check(fold, recs, n_reads, **kw)
    finally:
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


def star_read(read, first, count, edit=2):
    return [(read, 10 + first + k, edit) for k in range(count)]


# ---- 1. the worked example ----

@pytest.mark.parametrize("gname", list(GRAINS))
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_the_worked_example(iters, gname):
    rows, info, _ = run(GRAINS[gname], A.EXAMPLE, 4, w=W_HALF, slack=ALL, max_iters=iters, tol=0)
    masses, l1 = A.EXAMPLE_AFTER[iters - 1]
    assert dict(zip(rows["tax_id"].tolist(), rows["mass"].tolist())) == masses
    assert info["l1_change"] == l1 and info["iterations"] == iters and info["converged"] == 0
    assert {int(r["tax_id"]): (int(r["reads_any"]), int(r["reads_unique"])) for r in rows} == {5: (3, 1), 7: (2, 0), 9: (1, 1)}
    if iters == 3:
        assert (masses[5], masses[7], masses[9], l1) == (8077478865, 4807423021, 4294967296, 581047654)
        assert rows["assigned"].tolist() == [2, 1, 1] and info["total_mass"] == 17179869182 and info["reads"] == 4 and info["entries"] == 6


# ---- 2. tile sizes and grains ----

@pytest.mark.parametrize("tile", ["64", "1024"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_random_lists_at_both_tiles_and_all_grains(gname, tile, monkeypatch):
    monkeypatch.setenv("MTSV_ABUND_TILE", tile)
    rng = random.Random(3)
    pool = list(range(100, 160)) + [0, 77, 0x80000001, 4000000001]
    recs = random_list(rng, pool, 400, 60)
    if gname != "taxid":  # the wide grains repeat a TaxID inside a read, with different edits
        wide = []
        for read, t, e in recs:
            for gi in (1, 0x80000001, 9)[:rng.randrange(1, 4)]:
                for off in ((0, 9) if gname == "long" and rng.random() < 0.5 else (4,)):
                    wide.append((read, t, gi, off, e + rng.randrange(3) if gi > 1 else e))
        recs = wide
    assert len(recs) > 1500 and len({r[0] for r in recs}) > 250 and max(collections.Counter(r[0] for r in recs).values()) > 40
    for slack in (0, 1, ALL):
        run(GRAINS[gname], recs, 400, w=W_QUARTER, slack=slack, max_iters=4)


@pytest.mark.parametrize("gname", ["taxid_gi", "long"])
def test_a_run_of_one_taxid_over_several_tiles(gname, monkeypatch):
    # tile 64: read 1 has 150 records of one TaxID whose smallest edit is the last record's, then two more taxa
    monkeypatch.setenv("MTSV_ABUND_TILE", "64")
    recs = [(0, 5, 1, 0, 1), (0, 6, 1, 0, 2)] + [(1, 5, g, 1, 9 - (g == 150)) for g in range(1, 151)] + [(1, 6, 2, 2, 9), (1, 8, 2, 2, 8)]
    recs += [(2, 8, g, 0, 3) for g in range(1, 70)] + [(3, 5, 1, 1, 0)]
    _, info, want = run(GRAINS[gname], recs, 4, slack=0, max_iters=3)
    assert info["entries"] == 1 + 2 + 1 + 1 and want["assigned"][1] == (1, 5, 8)   # 5 and 8 tie at edit 8 for read 1 under slack 0


# ---- 3. where a read lies in its tile ----

@pytest.mark.parametrize("first_len", [62, 63, 64, 65, 66, 128, 129])
def test_a_read_that_ends_at_a_tile_edge(first_len, monkeypatch):
    # tile 64: the first read's last record at position 61 .. 65 (and 127, 128); behind it reads that lie inside the next tile
    monkeypatch.setenv("MTSV_ABUND_TILE", "64")
    recs = [(0, 10 + k, 2 + k % 3) for k in range(first_len)]
    for read in range(1, 40):
        recs += star_read(read, 7 * read, 1 + read % 4, edit=read % 3)
    recs += star_read(41, 100, 70) + star_read(42, 5, 1)
    run(M.GRAIN_TAXID, recs, 43, slack=1, max_iters=3)


# ---- 4. the read tiers ----

@pytest.mark.parametrize("lane_max", [None, "0", "1024", "3"])
def test_reads_at_the_tier_edges(lane_max, monkeypatch):
    if lane_max is not None:
        monkeypatch.setenv("MTSV_ABUND_LANE_MAX", lane_max)
    recs = []
    for read, count in enumerate((15, 16, 17, 1, 2, 3, 4, 63, 64, 65, 129, 1)):   # LANE_MAX - 1 .. + 1 at the default; wavefront-tier sizes
        recs += [(read, 10 + (5 * read + 3 * k) % 200, (read + k) % 4) for k in range(count)]
    assert len({(r, t) for r, t, _ in recs}) == len(recs)
    run(M.GRAIN_TAXID, recs, 12, w=W_QUARTER, slack=ALL, max_iters=4)
    run(M.GRAIN_TAXID, recs, 12, w=W_QUARTER, slack=1, max_iters=2)


def test_one_read_of_5000_taxa_among_200_short_ones():
    rng = random.Random(5)
    recs = random_list(rng, list(range(10, 5010)), 100, 6, skip=0)
    recs += [(100, 10 + k, k % 5) for k in range(5000)]
    recs += [(r + 1, t, e) for r, t, e in random_list(rng, list(range(10, 5010)), 200, 6, skip=0) if r >= 100]
    _, info, _ = run(M.GRAIN_TAXID, recs, 202, w=W_HALF, slack=ALL, max_iters=3)
    assert info["reads"] == 201 and info["entries"] == len(recs)


# ---- 5. the accumulation tiers ----

def test_global_adds_and_lds_adds_give_the_same_bytes(monkeypatch):
    recs = random_list(random.Random(6), list(range(50, 90)), 600, 30)
    results = []
    for dense in (None, "0"):
        if dense is not None:
            monkeypatch.setenv("MTSV_ABUND_DENSE_MAX", dense)
        fold = M.Fold(0, M.GRAIN_TAXID, n_reads=600)
        fold.add_records(as_array(M.GRAIN_TAXID, recs))
        out = M.Fold(0, M.GRAIN_TAXID)
        rows, info, _ = fold.abundance(W_QUARTER, max_iters=6, out=out)
        results.append((rows.tolist(), info, raw(out)))
        check(fold, recs, 600, w=W_QUARTER, max_iters=6)
        fold.close()
        out.close()
    assert results[0] == results[1]


@pytest.mark.parametrize("n_taxa", [8, 9])
def test_a_union_at_the_dense_edge(n_taxa, monkeypatch):
    monkeypatch.setenv("MTSV_ABUND_DENSE_MAX", "8")   # 8 TaxIDs: the last union that goes through LDS; 9: the first that does not
    recs = random_list(random.Random(7), list(range(20, 20 + n_taxa)), 300, n_taxa, skip=0.1)
    assert len({t for _, t, _ in recs}) == n_taxa
    _, info, _ = run(M.GRAIN_TAXID, recs, 300, max_iters=4)
    assert info["taxa"] == n_taxa


@pytest.mark.parametrize("dense", [None, "0"])
def test_one_taxon_in_every_one_of_20000_reads(dense, monkeypatch):
    if dense is not None:
        monkeypatch.setenv("MTSV_ABUND_DENSE_MAX", dense)
    rng = random.Random(8)
    recs = []
    for read in range(20000):
        recs.append((read, 9, rng.randrange(3)))
        if read % 3:
            recs.append((read, 10 + rng.randrange(30), rng.randrange(3)))
    rows, info, _ = run(M.GRAIN_TAXID, recs, 20000, w=W_HALF, max_iters=3, text=False)
    assert int(rows[0]["tax_id"]) == 9 and int(rows[0]["reads_any"]) == 20000 and info["reads"] == 20000
    assert int(rows[0]["mass"]) > info["total_mass"] // 2


# ---- 6. slack and weights ----

SLACK_RECS = [(0, 20, 2), (0, 21, 2), (0, 22, 3), (0, 23, 5), (0, 24, 9),          # one more taxon per slack
              (1, 21, 0xfffffffe), (1, 20, 0xffffffff), (1, 23, 0xfffffffc),      # edits at the top of the range
              (2, 24, 7),
              (3, 21, 0xffffffff), (3, 22, 0xffffffff),
              (4, 20, 0), (4, 22, 1), (4, 23, 4), (4, 24, 300),                   # d = 300: beyond every table
              (5, 20, 1), (5, 24, 2)]


@pytest.mark.parametrize("slack", [0, 1, 3, ALL])
def test_slack_values(slack, monkeypatch):
    monkeypatch.setenv("MTSV_ABUND_TILE", "64")
    want = A.entries(SLACK_RECS, slack)
    assert len(want[0]) == {0: 2, 1: 3, 3: 4, ALL: 5}[slack] and len(want[1]) == {0: 1, 1: 1, 3: 3, ALL: 3}[slack] and len(want[3]) == 2
    for grain in GRAINS.values():
        run(grain, SLACK_RECS, 6, w=W_HALF, slack=slack, max_iters=3)


@pytest.mark.parametrize("w", [[2 ** 31], [2 ** 31, 2 ** 29], [0], [2 ** 30, 0, 0, 5, 0], [2 ** 32 - 1] * 255],
                         ids=["n_w_1", "n_w_2", "a_zero", "zeros_inside", "n_w_255_of_ones"])
def test_a_difference_beyond_the_table_and_tables_with_zeros(w):
    _, _, want = run(M.GRAIN_TAXID, SLACK_RECS, 6, w=w, slack=ALL, max_iters=4)
    if w == [0]:   # a weight of zero: every read gives all of itself to its best taxa
        assert all(q in (0, 2 ** 32, 2 ** 31) for per in A.entries(SLACK_RECS, ALL).values() for q in A.shares(per, {t: 2 ** 32 for t in per}, w)[1].values())
        assert 6 * 2 ** 32 - 12 <= want["info"]["total_mass"] <= 6 * 2 ** 32      # (a share is truncated: a read of two may lose 2^-32)


# ---- 7. the uniform prior when every x is zero ----

@pytest.mark.parametrize("lane_max", [None, "0"])
def test_a_start_mass_of_one_takes_the_fallback_in_both_tiers(lane_max, monkeypatch):
    monkeypatch.setenv("MTSV_ABUND_START_MASS", "1")
    if lane_max is not None:
        monkeypatch.setenv("MTSV_ABUND_LANE_MAX", lane_max)
    recs = random_list(random.Random(10), list(range(30, 80)), 120, 40, skip=0.1)
    # every read of iteration 1 has s == 0 and takes the shares of the prior, W(d) >> 17
    ent = A.entries(recs, ALL)
    assert all(sum((1 * A.weight_of(d, W_HALF)) >> 48 for d, _ in per.values()) == 0 for per in ent.values())
    for iters in (0, 1, 3):
        run(M.GRAIN_TAXID, recs, 120, w=W_HALF, max_iters=iters, start=1)
    # weights of 3 and 1 times 2^16: 3 : 1 : 65536 under equal masses of 2^32, but 1 : 0 : 32768 under the prior -- another result
    small = [3 << 16, 1 << 16]
    assert A.run(recs, small, max_iters=1, start=1)["rows"] != A.run(recs, small, max_iters=1)["rows"]
    run(M.GRAIN_TAXID, recs, 120, w=small, max_iters=2, start=1)
    run(M.GRAIN_TAXID, recs, 120, w=[0, 0], max_iters=2, start=1)                  # the prior itself holds zeros


# ---- 8. stopping ----

def test_a_tol_that_stops_at_iteration_k_exactly():
    recs = random_list(random.Random(11), list(range(30, 50)), 200, 8, skip=0.1)
    history = A.run(recs, W_QUARTER, max_iters=6)["history"]
    l1 = [h[1] for h in history]
    k = 4
    assert l1[k - 1] > 0 and all(x > l1[k - 1] for x in l1[:k - 1])
    _, info, _ = run(M.GRAIN_TAXID, recs, 200, w=W_QUARTER, max_iters=6, tol=l1[k - 1])
    assert info["iterations"] == k and info["converged"] == 1 and info["l1_change"] == l1[k - 1]
    _, info, _ = run(M.GRAIN_TAXID, recs, 200, w=W_QUARTER, max_iters=6, tol=l1[k - 1] - 1)
    assert info["iterations"] > k and info["l1_change"] < l1[k - 1]
    _, info, _ = run(M.GRAIN_TAXID, recs, 200, w=W_QUARTER, max_iters=k, tol=l1[k - 1] - 1)   # the cap and no convergence
    assert info["iterations"] == k and info["converged"] == 0


def test_no_iteration_and_convergence_to_zero():
    recs = [(0, 7, 3), (0, 5, 3), (1, 9, 2), (1, 7, 1), (2, 5, 0)]
    rows, info, want = run(M.GRAIN_TAXID, recs, 3, max_iters=0)
    assert info["iterations"] == 0 and info["converged"] == 0 and info["l1_change"] == 0 and rows["mass"].tolist() == [2 ** 32] * 3
    assert want["assigned"] == [(0, 5, 3), (1, 7, 1), (2, 5, 0)]                    # by smallest edit, ties to the smallest TaxID
    single = [(r, 40 + r % 7, r % 3) for r in range(500)]                           # reads of one taxon each: A_1 = the counts, A_2 = A_1
    rows, info, _ = run(M.GRAIN_TAXID, single, 500, max_iters=50, tol=0)
    assert info["iterations"] == 2 and info["converged"] == 1 and info["l1_change"] == 0
    assert rows["mass"].tolist() == [n * 2 ** 32 for n in rows["reads_any"].tolist()] and rows["reads_unique"].tolist() == rows["reads_any"].tolist()


# ---- 9. ties, TaxIDs with bit 31 set, read numbers above 2^32 ----

def test_ties_go_to_the_smallest_taxid_as_unsigned():
    hi, top = 0x80000005, 0xfffffff0
    recs = [(0, hi, 1), (0, 7, 1), (0, top, 1),          # three taxa that are alike in every read: their masses stay equal
            (1, 7, 2), (1, hi, 2), (1, top, 2),
            (2, hi + 1, 0), (2, top + 1, 0),             # two more such, both with bit 31 set
            (3, 9, 4)]
    for grain in GRAINS.values():
        for iters in (0, 3):
            rows, _, want = run(grain, recs, 4, max_iters=iters)
            assert [t for _, t, _ in want["assigned"]] == [7, 7, hi + 1, 9]
            masses = dict(zip(rows["tax_id"].tolist(), rows["mass"].tolist()))
            assert masses[7] == masses[hi] == masses[top] and masses[hi + 1] == masses[top + 1]


def test_reads_numbered_above_2_to_32():
    n_reads = 2 ** 33 + 10
    recs = [(3, 9606, 1), (3, 9598, 1), (2 ** 32 - 1, 9606, 0), (2 ** 32, 9593, 0), (2 ** 32, 9606, 0), (2 ** 32 + 5, 9597, 2), (2 ** 33 + 1, 9606, 2),
            (2 ** 33 + 1, 63221, 1)]
    run(M.GRAIN_TAXID, recs, n_reads, max_iters=3, text=False)


# ---- 10. limits, refusals, fold states ----

def test_a_read_of_65535_taxa_passes_and_one_of_65536_is_refused():
    for count, ok in ((65535, True), (65536, False)):
        recs = [(0, 3, 1), (0, 4, 0)] + [(1, 100 + k, k % 2) for k in range(count)] + [(2, 5, 0)]
        fold = M.Fold(0, M.GRAIN_TAXID, n_reads=3)
        fold.add_records(as_array(M.GRAIN_TAXID, recs))
        out = M.Fold(0, M.GRAIN_TAXID, n_reads=2)
        out.add_records(as_array(M.GRAIN_TAXID, [(1, 5, 5)]))
        if ok:
            _, info, _ = check(fold, recs, 3, max_iters=1, out=out)
            assert info["entries"] == count + 3
        else:
            before = (raw(fold), raw(out), out.match_flags()[0].tobytes())
            with pytest.raises(M.MtsvError) as e:
                fold.abundance(W_HALF, max_iters=1, out=out)
            assert e.value.code == _lib.E_LIMIT and "65536" in str(e.value)
            assert (raw(fold), raw(out), out.match_flags()[0].tobytes()) == before
            with pytest.raises(OverflowError):
                A.run(recs, W_HALF, max_iters=1)
            check(fold, recs, 3, slack=0, max_iters=1, out=out)                     # half of them enter: legal
        fold.close()
        out.close()


def test_refusals_leave_both_folds_as_they_were(monkeypatch):
    L = M.lib()
    recs = [(0, 9606, 1), (0, 9598, 2), (3, 9598, 2)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=5)
    fold.add_records(as_array(M.GRAIN_TAXID, recs))
    wide = M.Fold(0, M.GRAIN_LONG, n_reads=4)
    wide.add_records(as_array(M.GRAIN_LONG, [(2, 5, 5)]))
    narrow = M.Fold(0, M.GRAIN_TAXID, n_reads=4)
    narrow.add_records(as_array(M.GRAIN_TAXID, [(2, 5, 5)]))
    state = lambda: [(f.count(), raw(f), f.match_flags()[0].tobytes()) for f in (fold, wide, narrow)]  # noqa: E731
    before = state()
    w = np.array(W_HALF, dtype="<u4")
    ptr, n, info = C.c_void_p(), C.c_uint64(), M.AbundanceInfo()

    def refused(f, wp, n_w, out, rows=None, n_rows=None, code=_lib.E_ARG):
        rc = L.mtsv_fold_abundance(f, wp, n_w, ALL, 3, 0, out, rows, n_rows, C.byref(info), None)
        assert rc == code, L.mtsv_last_error()
        assert state() == before and ptr.value is None

    refused(None, w.ctypes.data, 64, narrow.h)                                        # a null f
    refused(fold.h, None, 64, narrow.h)                                               # a null w
    refused(fold.h, w.ctypes.data, 0, narrow.h)                                       # n_w outside 1 .. 255
    refused(fold.h, w.ctypes.data, 256, narrow.h)
    refused(fold.h, w.ctypes.data, 64, fold.h)                                        # out == f
    refused(fold.h, w.ctypes.data, 64, wide.h)                                        # out of a wide grain
    refused(wide.h, w.ctypes.data, 64, wide.h)
    refused(fold.h, w.ctypes.data, 64, narrow.h, rows=C.byref(ptr))                   # rows without n_rows
    if M.device_count() > 1:
        far = M.Fold(1, M.GRAIN_TAXID, n_reads=4)
        refused(fold.h, w.ctypes.data, 64, far.h)                                     # another device
        far.close()
    # a refused device allocation, on each of the two named arrays
    for what in ("the abundance entries", "the abundance masses"):
        monkeypatch.setenv("MTSV_ALLOC_REFUSE", what)
        fresh = M.Fold(0, M.GRAIN_TAXID, n_reads=5)                                   # (a fold that has not made its arrays yet)
        fresh.add_records(as_array(M.GRAIN_TAXID, recs))
        seen = raw(fresh)
        rc = L.mtsv_fold_abundance(fresh.h, w.ctypes.data, 64, ALL, 3, 0, narrow.h, C.byref(ptr), C.byref(n), C.byref(info), None)
        assert rc not in (0, _lib.E_ARG) and what in L.mtsv_last_error().decode() and ptr.value is None
        assert state() == before and raw(fresh) == seen
        monkeypatch.delenv("MTSV_ALLOC_REFUSE")
        check(fresh, recs, 5, out=narrow)                                             # and the same call works afterwards
        fresh.close()
        narrow.reset(4)
        narrow.add_records(as_array(M.GRAIN_TAXID, [(2, 5, 5)]))
    check(fold, recs, 5, out=narrow)
    for f in (fold, wide, narrow):
        f.close()


def test_an_output_fold_that_must_grow():
    n = 70000                                                                         # above the first allocation of a fold
    recs = [(r, (9606, 9598, 9593)[r % 3], r % 5) for r in range(n)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=n)
    fold.add_records(as_array(M.GRAIN_TAXID, recs))
    out = M.Fold(0, M.GRAIN_TAXID, n_reads=2)
    out.add_records(as_array(M.GRAIN_TAXID, [(1, 5, 5)]))
    rows, info, _ = fold.abundance(W_HALF, max_iters=2, out=out)
    got = out.download()
    assert info["reads"] == n and np.array_equal(got["read"], np.arange(n)) and got["tax_id"].tolist() == [r[1] for r in recs]
    assert got["edit"].tolist() == [r[2] for r in recs]
    assert rows["assigned"].tolist() == [23333, 23333, 23334] and rows["mass"].tolist() == [23333 * 2 ** 32, 23333 * 2 ** 32, 23334 * 2 ** 32]
    assert len(out.match_flags()[0]) == n
    fold.close()
    out.close()


def test_an_empty_fold():
    fold = M.Fold(0, M.GRAIN_TAXID_GI, n_reads=9)
    out = M.Fold(0, M.GRAIN_TAXID, n_reads=3)
    out.add_records(as_array(M.GRAIN_TAXID, [(1, 5, 5)]))
    rows, info, ms = fold.abundance(W_HALF, out=out)
    assert len(rows) == 0 and ms == 0 and info == dict(reads=0, entries=0, taxa=0, total_mass=0, l1_change=0, iterations=0, converged=0)
    assert out.count() == 0 and len(out.download()) == 0
    flags, matched = out.match_flags()
    assert len(flags) == 9 and matched == 0                                           # as after mtsv_fold_reset(out, 9)
    assert out.format_text(ids_of(9))[0] == b"" and len(out.taxa_report()[0]) == 0
    assert M.format_abundance(rows, info) == A.HEADER.encode()
    fold.close()
    out.close()


def test_a_second_call_after_new_taxids_were_folded_in(monkeypatch):
    monkeypatch.setenv("MTSV_ABUND_TILE", "64")
    first = [(0, 9606, 1), (0, 9598, 1), (2, 9597, 0)]
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=6)
    out = M.Fold(0, M.GRAIN_TAXID)
    fold.add_records(as_array(M.GRAIN_TAXID, first))
    check(fold, first, 6, out=out)
    more = [(0, 9593, 1), (3, 77, 0), (4, 9583, 2), (4, 9606, 2)]                     # a new TaxID for read 0, new reads
    fold.add_records(as_array(M.GRAIN_TAXID, more))
    both = sorted(first + more)
    _, info, _ = check(fold, both, 6, out=out)                                        # the same output fold again
    assert info["taxa"] == 6 and info["reads"] == 4
    big = M.Fold(0, M.GRAIN_TAXID, n_reads=100000)                                    # an output fold that holds more than it gets
    big.add_records(as_array(M.GRAIN_TAXID, [(r, 9606, 0) for r in range(70000)]))
    check(fold, both, 6, out=big)
    for f in (fold, out, big):
        f.close()


# ---- 11. the command line ----

def abund_tool(tmp_path, texts, *extra, env=None, tag="ab"):
    table, lines = tmp_path / f"{tag}.abundance", tmp_path / f"{tag}.reassigned"
    r, out, rep = PC.run_tool(tmp_path, texts, "--on-gpu", "--abundance", str(table), "--reassigned", str(lines), *extra, env=env, tag=tag)
    return r, out, rep, (table.read_bytes() if table.exists() else None), (lines.read_bytes() if lines.exists() else None)


@pytest.mark.parametrize("case", ["default/taxid", "long/taxid-gi"])
def test_cli_golden_results_cut_into_three_files(case, tmp_path):
    name, mode = case.split("/")
    texts = PC.golden_cut("e2e_default.results" if name == "default" else "e2e_default_long.results")
    plain, plain_out, plain_rep = PC.run_tool(tmp_path, texts, "--mode", mode, "--on-gpu", tag="plain")
    assert plain.returncode == 0, plain.stderr
    ids, recs = P.collapse_files(P.TAXID if mode == "taxid" else P.TAXID_GI, texts)
    # at the defaults
    r, out, rep, table, lines = abund_tool(tmp_path, texts, "--mode", mode)
    assert r.returncode == 0, r.stderr
    assert out == plain_out and rep == plain_rep and len(out) > 0 and len(rep) > 0    # -o and --report: what they are without
    want = A.run(recs, W_QUARTER, slack=ALL, max_iters=100, tol=TOL_DEFAULT)
    assert want["info"]["converged"] == 1 and want["info"]["iterations"] < 100 and want["info"]["reads"] == len(out.splitlines()) > 100
    assert table == A.tsv(want["rows"], want["info"]["total_mass"])
    assert lines == A.lines(want["assigned"], ids)
    assert [l.split(b":")[0] for l in lines.splitlines()] == [l.rsplit(b":", 1)[0] for l in out.splitlines()]  # the order of -o's lines
    # with every option
    r, out2, _, table2, lines2 = abund_tool(tmp_path, texts, "--mode", mode, "--abundance-mismatch", "0.5", "--abundance-slack", "1", "--abundance-iters", "3",
                                            tag="opts")
    assert r.returncode == 0, r.stderr
    want2 = A.run(recs, W_HALF, slack=1, max_iters=3, tol=TOL_DEFAULT)
    assert want2["info"]["iterations"] == 3 and out2 == plain_out
    assert table2 == A.tsv(want2["rows"], want2["info"]["total_mass"]) and table2 != table
    assert lines2 == A.lines(want2["assigned"], ids)
    # a tolerance given in reads, and the table alone
    only = tmp_path / "only.abundance"
    r, _, _ = PC.run_tool(tmp_path, texts, "--mode", mode, "--on-gpu", "--abundance", str(only), "--abundance-tol", "2.5", "--abundance-slack", "all", tag="one")
    want3 = A.run(recs, W_QUARTER, slack=ALL, max_iters=100, tol=int(2.5 * 2 ** 32))
    assert r.returncode == 0 and only.read_bytes() == A.tsv(want3["rows"], want3["info"]["total_mass"]) and not (tmp_path / "one.reassigned").exists()
    assert want3["info"]["iterations"] < want["info"]["iterations"]


def test_cli_usage_errors(tmp_path):
    texts = ["a:2=1,3=1\n"]

    def usage(*args):
        r, out, _ = PC.run_tool(tmp_path, texts, *args, tag="usage")
        assert r.returncode == 1 and out is None and r.stderr.startswith("error: "), (args, r.stderr)
        assert not list(tmp_path.glob("*.abundance")) and not list(tmp_path.glob("*.reassigned"))
        return r.stderr

    table, lines = str(tmp_path / "u.abundance"), str(tmp_path / "u.reassigned")
    assert "'--abundance <TSV>' requires '--on-gpu'" in usage("--abundance", table)
    assert "'--reassigned <PATH>' requires '--abundance <TSV>'" in usage("--on-gpu", "--reassigned", lines)
    assert "'--abundance-mismatch <Q>' requires '--abundance <TSV>'" in usage("--on-gpu", "--abundance-mismatch", "0.5")
    assert "'--abundance-slack <N|all>' requires '--abundance <TSV>'" in usage("--on-gpu", "--abundance-slack", "2")
    assert "'--abundance-iters <N>' requires '--abundance <TSV>'" in usage("--on-gpu", "--abundance-iters", "2")
    assert "'--abundance-tol <READS>' requires '--abundance <TSV>'" in usage("--on-gpu", "--abundance-tol", "0.5")
    for bad in ("0", "1.5", "-0.25", "nan", "half", ""):
        assert f"Invalid value for '--abundance-mismatch <Q>': {bad}" in usage("--on-gpu", "--abundance", table, "--abundance-mismatch", bad)
    assert "Invalid value for '--abundance-slack <N|all>': some" in usage("--on-gpu", "--abundance", table, "--abundance-slack", "some")
    assert "Invalid value for '--abundance-iters <N>': -1" in usage("--on-gpu", "--abundance", table, "--abundance-iters", "-1")
    for bad in ("-1", "nan", "1e30", "x"):
        assert f"Invalid value for '--abundance-tol <READS>': {bad}" in usage("--on-gpu", "--abundance", table, "--abundance-tol", bad)


@pytest.mark.parametrize("case", ["key_order", "no_offset"])
def test_cli_refused_input_with_abundance_ends_non_zero(case, tmp_path):
    texts = {"key_order": PC.KEY_ORDER, "no_offset": PC.NO_OFFSET}[case]
    r, out, rep, table, lines = abund_tool(tmp_path, texts, "--mode", "taxid-gi")
    assert r.returncode not in (0, 1) and table is None and lines is None and out is None, r.stderr
    assert "--on-gpu:" in r.stderr and "--abundance needs the device path" in r.stderr
    h, h_out, _ = PC.run_tool(tmp_path, texts, "--mode", "taxid-gi", "--on-gpu", tag="fallback")   # without --abundance the host path takes it
    assert h.returncode == 0 and len(h_out) > 0
