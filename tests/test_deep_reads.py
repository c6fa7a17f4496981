"""-m gpu tests of reads that carry thousands of hits through merge, collapse, report, flags and fold (k_merge.hip,
k_collapse.hip, k_report.hip, k_match.hip, k_fold.hip).  The cases are deep_cases.py's (test_deep_reads_cpu.py shows from the
oracle alone what each holds): up to 64 small chunk databases, each run in a workspace of its own over the same reads and
merged, give per-read hit lists of 640 to 8192 hits -- the second and later trips of block_bitonic's stride loop, the LDS
tier's edges at the default thresholds (4096 | 4097 keys, 2048 | 2049 wide keys), the global tier with and without skipped
upper indexes, the source limit of mtsv_batch_merge_runs, reads that own several fold tiles of 1024 -- and wide_chunk gives
more than 512 hits on both strands in the layout of a single pass.

Expected values never come from the device: the oracle's hits per chunk, merged by chunk_merge_ref.merge_hits, restated by
assign_ref / grain_ref / taxa_report_ref / fold_ref.  Every comparison is exact.  The oracle's hits and what is restated from
them are computed once per process and shared; every source workspace runs once per grain and is shared by the tests."""
import numpy as np
import pytest

import assign_ref as A
import chunk_merge_ref as CM
import deep_cases as D
import grain_ref as GR
import mtsv_tools_amd as M
import taxa_report_ref as R
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from test_assignment_grains import expected_tiers, set_edges, traced_tiers
from test_fold import check_fold

pytestmark = pytest.mark.gpu

GRAINS = {"taxid": (M.GRAIN_TAXID, A.collapse, ""), "taxid_gi": (M.GRAIN_TAXID_GI, GR.collapse_taxid_gi, " [grain taxid-gi]"),
          "long": (M.GRAIN_LONG, GR.collapse_long, " [grain long]")}
MERGED = [c for c in D.CASES if c != "one_pass"]
LDS_KEYS = {"taxid": 4096, "taxid_gi": 2048, "long": 2048}
WS_HITS = 1 << 18          # seed hits of a source's workspace: 66 of them stay cheap, a source takes a pass or two
FOLD_TILE = 1024
N_DEEP = len(D.DEEP)
LDS, GLOBAL = 2, 3         # places in the traced tier counts


def records(b, gname):
    if gname == "taxid":
        a, ms = b.download_assignments()
        return A.as_triples(a)
    a, ms = b.download_assignments_gi()
    return GR.as_tuples(a)


def raw_records(x, gname):
    """the bytes of a collector's or a fold's records"""
    if isinstance(x, M.Fold):
        return (x.download() if gname == "taxid" else x.download_gi()).tobytes()
    return (x.download_assignments()[0] if gname == "taxid" else x.download_assignments_gi()[0]).tobytes()


_want = {}


def want_records(case, gname):
    if (case, gname) not in _want:
        _want[case, gname] = GRAINS[gname][1](D.merged(case))
    return _want[case, gname]


class World:
    """the chunk indexes on the device and one workspace per chunk with the reads resident (uploaded to the first, copied to
    the others), made when first asked for; a source is run plainly, or with the assignments on in a grain (it keeps its
    hits, so it stays a source of merges), and run again only when another grain is asked for"""

    def __init__(self):
        self.bases, self.off = D.batch()
        self.n = len(D.READS)
        self.ixs, self.srcs, self.grain = {}, {}, {}
        self.first = None

    def index(self, key):
        if key not in self.ixs:
            ix = M.MGIndex.build(D.entries_of(key), threads=4)
            ix.to_device(0)
            self.ixs[key] = ix
        return self.ixs[key]

    def source(self, key, gname=None):
        if key not in self.srcs:
            b = M.Batch(self.index(key), 0, self.n, len(self.bases), max_hits_ws=WS_HITS)
            if self.first is None:
                b.upload(self.bases, self.off)
                self.first = b
            else:
                assert b.copy_reads(self.first) >= 0.0
            b.run()
            self.srcs[key], self.grain[key] = b, None
        b = self.srcs[key]
        if self.grain[key] != gname:
            b.set_assignments(M.ASSIGN_OFF)
            if gname is not None:
                b.set_assignment_grain(GRAINS[gname][0])
                b.set_assignments(M.ASSIGN_WITH_HITS)
            b.run()
            self.grain[key] = gname
        return b

    def sources(self, case, gname=None):
        """the case's sources in merge order; gname: each with the assignments of its own run on in that grain"""
        if gname is None:
            return [self.srcs[k] if k in self.srcs else self.source(k) for k in D.chunk_keys(case)]
        return [self.source(k, gname) for k in D.chunk_keys(case)]

    def collector(self, gname=None, mode=M.ASSIGN_ONLY, flags=False, report=False):
        dst = M.Batch(self.index(("full", 0)), 0, 64, 1 << 12)
        if flags:
            dst.set_match_flags(M.MATCH_WITH_HITS)
        if report:
            dst.set_taxa_report(True)
        if gname is not None:
            dst.set_assignment_grain(GRAINS[gname][0])
            dst.set_assignments(mode)
        return dst

    def close(self):
        for x in list(self.srcs.values()) + list(self.ixs.values()):
            x.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def report_of(b):
    rows, total, ms = b.taxa_report()
    assert list(rows["tax_id"]) == sorted(set(rows["tax_id"].tolist())) and ms >= 0
    return R.rows_dict(rows), total


def check_flags(b, hits, n):
    flags, n_matched = b.match_flags()
    pres = CM.presence(hits, n)
    assert len(flags) == n and np.array_equal(flags, pres) and n_matched == int(pres.sum())


# ---- 1. the merge, hit for hit, and its flags ----

@pytest.mark.parametrize("case", MERGED)
def test_merged_hits_and_flags_equal_the_restatement(world, case):
    want = D.merged(case)
    counts = D.want_counts(case)
    per_read = D.per_read(want)
    assert {int(per_read[r]) for r in D.DEEP} == set(counts.values())        # (test_deep_reads_cpu.py has the whole of it)
    srcs = world.sources(case)
    dst = world.collector(flags=True)
    assert dst.merge_runs(srcs) >= 0.0
    assert_same_hits(dst.download(), want)
    st = dst.stats()
    assert (st["n_reads"], st["n_hits"]) == (world.n, len(want))
    check_flags(dst, want, world.n)
    dst.close()


# ---- 2. the collapse of the merge in every grain, tier by tier ----

@pytest.mark.parametrize("gname", list(GRAINS))
@pytest.mark.parametrize("case", MERGED)
def test_collector_records_and_tiers(world, case, gname, monkeypatch, capfd):
    grain, restate, suffix = GRAINS[gname]
    hits = D.merged(case)
    want = want_records(case, gname)
    counts = D.want_counts(case)
    lds_keys = LDS_KEYS[gname]
    srcs = world.sources(case)
    monkeypatch.setenv("MTSV_TRACE", "1")

    def through(env, lds_max):
        set_edges(monkeypatch, env)
        dst = world.collector(gname)                                          # (the tier edges are read as the assignments are switched on)
        capfd.readouterr()
        dst.merge_runs(srcs)
        got = records(dst, gname)
        tiers, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err, suffix, "merge")
        dst.close()
        assert got == want, env
        assert (n_hits, n_assign) == (len(hits), len(want))
        assert edges == (16, 64, lds_max), env
        assert tiers == expected_tiers(hits, world.n, *edges), env
        assert tiers[1] == 0 and tiers[LDS] + tiers[GLOBAL] == N_DEEP         # every deep read is a listed one
        return tiers

    if case == "moved_edge":
        assert counts["in"] == counts["out"] == 1024
        t = through({"LDS_MAX": 1024}, 1024)                                  # n = lds_max exactly: the last read of the LDS tier
        assert t[LDS] == N_DEEP
        t = through({"LDS_MAX": 512}, 512)                                    # the same reads sort in global memory
        assert t[GLOBAL] == N_DEEP
        return
    t = through({}, lds_keys)
    want_lds = sum(counts[k] <= lds_keys for k in D.KINDS if k in counts)
    assert t[LDS] == want_lds
    if case == "two_trips":
        assert t[LDS] == N_DEEP
    elif case == "wide_edge":
        assert t[LDS] == (N_DEEP if gname == "taxid" else N_DEEP // 2)        # 2048 | 2049 wide keys
    elif case == "taxid_edge":
        assert t[LDS] == (N_DEEP // 2 if gname == "taxid" else 0)             # 4096 | 4097 keys
    else:
        assert t[GLOBAL] == N_DEEP


# ---- 3. the report of the merge, dense and hashed ----

@pytest.mark.parametrize("dense_max", [None, "1"], ids=["dense", "hashed"])
@pytest.mark.parametrize("case", MERGED)
def test_report_of_the_merge(world, case, dense_max, monkeypatch):
    """the cooperative walk of k_report (64 hits a step, two sweeps) is quadratic in a read's hits.  Measured on an MI355X,
    the report kernel of one merge of these 24 deep reads: 640 hits 7 ms, 2048 61 ms, 4096 242 ms, 5120 0.37 s, 8192 0.95 s,
    dense and hashed alike -- so the two deepest cases are in"""
    if dense_max:
        monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", dense_max)
    else:
        monkeypatch.delenv("MTSV_REPORT_DENSE_MAX", raising=False)
    want = D.merged(case)
    dst = world.collector(report=True)
    dst.merge_runs(world.sources(case))
    assert report_of(dst) == R.classify_hits(want)
    dst.close()


# ---- 4. the fold of the collector: records, report (k_fold_report) and flags ----

@pytest.mark.parametrize("gname", list(GRAINS))
@pytest.mark.parametrize("case", MERGED)
def test_fold_of_the_collector(world, case, gname, monkeypatch):
    set_edges(monkeypatch, {"LDS_MAX": D.CASES[case][2]} if D.CASES[case][2] else {})
    want = want_records(case, gname)
    dst = world.collector(gname)
    dst.merge_runs(world.sources(case))
    fold = M.Fold(0, GRAINS[gname][0], n_reads=world.n)
    assert fold.add_run(dst) >= 0.0
    check_fold(fold, want, world.n)
    rows, total, _ = fold.taxa_report()
    assert (R.rows_dict(rows), total) == R.classify_hits(D.merged(case))      # ... which is the classification of the hits
    assert raw_records(fold, gname) == raw_records(dst, gname)
    fold.close()
    dst.close()


def tile_edges_inside_a_read(recs, tile=FOLD_TILE):
    """the most tile edges that fall between two records of one read, in a list laid out in tiles of `tile` records"""
    first, last = {}, {}
    for i, r in enumerate(recs):
        first.setdefault(r[0], i)
        last[r[0]] = i
    return max(last[r] // tile - first[r] // tile for r in first)


@pytest.mark.parametrize("gname", list(GRAINS))
@pytest.mark.parametrize("case", ["two_trips", "taxid_edge", "full_house"])
def test_sources_folded_one_at_a_time_in_both_orders(world, case, gname, monkeypatch):
    set_edges(monkeypatch, {})
    monkeypatch.delenv("MTSV_FOLD_TILE", raising=False)                        # the default tile of 1024
    grain = GRAINS[gname][0]
    want = want_records(case, gname)
    # from the expected list: a read's records lie on both sides of a tile edge; in full_house the more than 5000 records of a
    # read of the long grain lie across five edges and more
    assert tile_edges_inside_a_read(want) >= (5 if (case, gname) == ("full_house", "long") else 1)
    srcs = world.sources(case, gname)
    dst = world.collector(gname)
    dst.merge_runs(srcs)
    raw = raw_records(dst, gname)
    dst.close()
    assert len(raw) == len(want) * (16 if gname == "taxid" else 24)
    fold = M.Fold(0, grain)
    for order in (srcs, srcs[::-1]):
        fold.reset(world.n)
        for b in order:
            assert fold.add_run(b) >= 0.0
        assert raw_records(fold, gname) == raw
        check_fold(fold, want, world.n)
    fold.close()


# ---- 5. the layout of a pass: both strand slots of a read filled ----

@pytest.mark.parametrize("gname", list(GRAINS))
def test_one_pass_of_more_than_512_hits_on_both_strands(world, gname, monkeypatch, capfd):
    grain, restate, suffix = GRAINS[gname]
    hits = D.merged("one_pass")
    want = want_records("one_pass", gname)
    per_read = D.per_read(hits)
    for r in D.DEEP:
        fwd, rev = D.strand_counts(hits, r)
        assert fwd > 0 and rev > 0 and fwd + rev == per_read[r] > 512
    ix = world.index(("wide",))
    set_edges(monkeypatch, {})
    monkeypatch.setenv("MTSV_TRACE", "1")
    for dense_max in (None, "1"):
        if dense_max:
            monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", dense_max)
        else:
            monkeypatch.delenv("MTSV_REPORT_DENSE_MAX", raising=False)
        b = M.Batch(ix, 0, world.n, len(world.bases))
        b.set_assignment_grain(grain)
        b.set_assignments(M.ASSIGN_WITH_HITS)
        b.set_taxa_report(True)
        b.set_match_flags(M.MATCH_WITH_HITS)
        b.upload(world.bases, world.off)
        capfd.readouterr()
        b.run()
        tiers, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err, suffix)
        assert_same_hits(b.download(), hits)
        assert records(b, gname) == want
        assert tiers == expected_tiers(hits, world.n, *edges) and tiers[LDS] == N_DEEP and (n_hits, n_assign) == (len(hits), len(want))
        assert report_of(b) == R.classify_hits(hits)
        check_flags(b, hits, world.n)
        fold = M.Fold(0, grain, n_reads=world.n)
        fold.add_run(b)
        check_fold(fold, want, world.n)
        fold.close()
        b.close()
    # run_host on one lane
    monkeypatch.delenv("MTSV_REPORT_DENSE_MAX", raising=False)
    b = M.Batch(ix, 0, world.n, len(world.bases), lanes=1)
    b.set_assignment_grain(grain)
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.set_taxa_report(True)
    b.set_match_flags(M.MATCH_WITH_HITS)
    b.run_host(world.bases, world.off)
    assert b.stats()["n_lanes"] == 1
    assert_same_hits(b.download(), hits)
    assert records(b, gname) == want
    assert report_of(b) == R.classify_hits(hits)
    check_flags(b, hits, world.n)
    b.close()


# ---- 6. the source limit ----

def test_a_65th_source_is_refused_and_the_collector_keeps_the_merge_of_64(world):
    case = "full_house"
    want = D.merged(case)
    recs = want_records(case, "long")
    srcs = world.sources(case)
    assert len(srcs) == 64
    dst = world.collector("long", mode=M.ASSIGN_WITH_HITS, flags=True, report=True)
    dst.merge_runs(srcs)
    report = R.classify_hits(want)
    assert records(dst, "long") == recs and report_of(dst) == report         # (k_report over reads of 8192 hits: once, here)
    extra = world.source(("unit",))
    with pytest.raises(M.MtsvError) as e:
        dst.merge_runs(srcs + [extra])
    assert e.value.code == _lib.E_ARG
    assert_same_hits(dst.download(), want)                                     # what the merge of 64 left
    assert records(dst, "long") == recs
    assert report_of(dst) == report
    check_flags(dst, want, world.n)
    assert dst.stats()["n_hits"] == len(want)
    dst.merge_runs(srcs[:5] + [extra])                                         # ... and it still takes a merge
    assert_same_hits(dst.download(), CM.merge_hits(D.parts("two_trips") + [D.oracle_part(("unit",))]))
    dst.close()
