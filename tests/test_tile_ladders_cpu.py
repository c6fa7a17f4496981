"""CPU tests of tile_cases.py: the cases built onto the structural edges of the tiled passes hold what they claim, for every
tile of every ladder.  A generator that misses a side of an edge fails here, not silently on the device.  Nothing here runs
library code beyond the record dtypes: coverage is computed from the lists, expectations from the restatements."""
import numpy as np
import pytest

import abund_ref as AR
import fold_ref as F
import lca_ref as R
import pair_ref as PR
import parse_ref as P
import text_cases as TC
import tile_cases as K

GRAINS = TC.GRAINS
ALL = 0xffffffff


def test_kinds_and_edges():
    assert [K.kinds(T) for T in K.LCA_TILES] == [[64], [64, 128], [64, 256], [2, 128, 512], [4, 256, 1024]]
    assert K.kinds(2, ceil=True) == [64, 2] and K.kinds(512, ceil=True) == [2, 128, 512]
    assert [K.kinds(T) for T in K.PARSE_TILES] == [[64], [64, 256], [4, 256, 1024], [16, 1024, 4096], [32, 2048, 8192], [64, 4096, 16384]]
    assert K.targets(1024, -1) == [3, 255, 1023, 1027, 1279, 2047]
    assert K.targets(1024, 0, floor=64) == [64, 256, 1024, 1088, 1280, 2048]
    assert K.missing({p + d for p in K.targets(1024, 0) for d in K.SIDES}, 1024) == []
    assert K.missing({p + d for p in K.targets(1024, 0) for d in (-1, 0)}, 1024) == [(E, 1, w) for E in (4, 256, 1024) for w in ("first", "later")]
    assert (4, 0, "later") in K.missing({3, 4, 5, 1023, 1024, 1025}, 1024)          # 1024 is no edge behind the first tile


# ---- LCA ----

@pytest.fixture(scope="module")
def outlier():
    return R.Taxonomy(K.OUTLIER)


def test_the_outlier_taxonomy(outlier):
    tx = outlier
    assert (len(K.FILLERS), len(K.LOWS), len(K.HIGHS)) == (3000, 375, 375)
    assert tx.parent_of(100) == 1 and [tx.parent_of(t) for t in (50, 60, 70)] == [100] * 3
    assert all(K.FILLERS[0] < x < K.FILLERS[-1] for x in K.LOWS + K.HIGHS)           # the outliers' TaxIDs fall between fillers'
    assert tx.lca([1000, 1001]) == 60 and tx.lca([1000, 1003, 1004]) == 100 and tx.lca([1000, 1007]) == 100 and tx.lca([1003]) == 1003
    # preorder, children ascending by TaxID: 50's subtree lies below every filler, 70's above
    for taxa in ([1001, 1003, 1004], [1005, 1006, 1007]):
        assert tx.lca_by_intervals(taxa) == 100


@pytest.mark.parametrize("T", K.LCA_TILES)
def test_lca_cases_hold_what_they_claim(T, outlier):
    tx = outlier
    cases = K.lca_cases(T)
    union = {"heads": set(), "b": set(), "c": set(), "d": set()}
    for name, (recs, n_reads) in cases.items():
        assert recs == sorted(recs) and len({r[:2] for r in recs}) == len(recs) and recs[-1][0] < n_reads, name
        assert 200 <= len(recs) <= max(3 * T + 50, 300), (name, len(recs))
        ev = K.lca_events(recs)
        if name[:-2] in ("heads", "b", "c", "d"):
            kind, d = name[:-2], int(name[-2:])
            assert set(K.targets(T, d)) <= ev[kind], name
            union[kind] |= ev[kind] if kind != "heads" else set(K.targets(T, d)) & ev[kind]
            if kind == "heads":                                                    # the side alone: no head next to the edge but this one
                assert all(p + e not in ev["heads"] for p in K.targets(T, d) for e in (-1, 1) if p + e > 0), name
        # what the events mean, by the restatement: the smallest edit alone enters at slack 0; an outlier lifts the LCA to 100
        # and 60 is what is left without it
        at0 = {r: t for r, t, _ in R.per_read(tx, recs, 0)}
        everything = {r: t for r, t, _ in R.per_read(tx, recs, ALL)}
        for i, j in K.reads_of(recs):
            read = recs[i][0]
            for p in range(i, j):
                if p in ev["b"]:
                    assert at0[read] == recs[p][1], name
                    assert R.per_read(tx, recs[i:p] + recs[p + 1:j], 0)[0][1] != recs[p][1]
                if p in ev["c"] or p in ev["d"]:
                    assert everything[read] == 100, name
                    assert R.per_read(tx, recs[i:p] + recs[p + 1:j], ALL)[0][1] in (60, recs[i][1], recs[j - 1][1]), name
    for kind, got in union.items():
        assert K.missing(got, T) == [], kind
    # the reads measured against a wavefront span
    S = K.lca_span(T)
    reads = K.reads_of(cases["spans"][0])
    assert {(0, S - 1), (S - 1, S), (S, 2 * S), (2 * S, 2 * S + 1), (2 * S + 1, 3 * S)} <= set(reads)
    ev = K.lca_events(cases["spans"][0])
    assert {S // 2, 2 * S - 1, 2 * S + 1} <= ev["b"] and {S - 2, S} <= ev["c"] and 3 * S - 1 in ev["d"]
    # the read longer than two tiles: its smallest edit and its outlier in every pair of neighbouring tiles of its three
    seen = set()
    for rot in range(3):
        for k in "cd":
            recs = cases[f"long{rot}{k}"][0]
            (i, j), = [(i, j) for i, j in K.reads_of(recs) if j - i > 2 * T]
            assert i // T == 0 and (j - 1) // T == 2
            ev = K.lca_events(recs)
            (b,), (o,) = [p for p in ev["b"] if i <= p < j], [p for p in ev[k] if i <= p < j]
            seen.add((k, b // T, o // T))
    assert seen == {(k, t, (t + 1) % 3) for k in "cd" for t in range(3)}


def test_lca_expectations_pinned_by_hand_at_tile_64(outlier):
    """the three lists of side 0 at tile 64: the edges are 64 and 128, the reads [0, 96), [96, 200) hold one event each"""
    cases = K.lca_cases(64)
    for kind in "bcd":
        recs, _ = cases[f"{kind}+0"]
        assert K.reads_of(recs) == [(0, 96), (96, 200)]
        at0, everything = R.per_read(outlier, recs, 0), R.per_read(outlier, recs, ALL)
        assert [t for _, t, _ in everything] == ([60, 60] if kind == "b" else [100, 100])
        if kind == "b":
            assert [t for _, t, _ in at0] == [recs[64][1], recs[128][1]]
        else:
            assert K.leaf_parent(recs[64][1]) == K.leaf_parent(recs[128][1]) == (50 if kind == "c" else 70)
            assert all(K.leaf_parent(t) == 60 for _, t, _ in at0)                   # the smallest edit is a filler's
    recs, _ = cases["heads+0"]
    assert K.reads_of(recs) == [(0, 64), (64, 128), (128, 200)]


# ---- runs: pairs and abundance ----

def is_wide_list(recs, n_reads, vary):
    """a list at the LONG grain, with vary 'gi' at the TAXID_GI grain as well"""
    return (recs == sorted(recs) and len({r[:4 if vary == "offset" else 3] for r in recs}) == len(recs)
            and recs[-1][0] < n_reads and n_reads % 2 == 0 and max(r[4] for r in recs) < 2 ** 31)


@pytest.mark.parametrize("vary", ["offset", "gi"])
@pytest.mark.parametrize("T", K.PAIR_TILES)
def test_run_cases_hold_what_they_claim(T, vary):
    assert K.PAIR_TILES == K.ABUND_TILES == K.LCA_TILES                              # the same edges: K.targets(T, d)
    at_reads, at_runs, joined = set(), set(), 0
    for name, (recs, n_reads) in K.run_cases(T, vary).items():
        tg = set(K.targets(T, int(name[-2:])))
        assert is_wide_list(recs, n_reads, vary) and 200 <= len(recs) <= max(3 * T + 50, 300), name
        reads, runs = K.run_heads_of(recs)
        if name.startswith("reads"):                                                # the side alone: no head but at the edges
            assert reads == tg | {0} and runs == set(range(len(recs))), name
            assert F.is_list(F.TAXID, K.narrow(recs)), name
            at_reads |= tg
            joined += len(PR.pair(PR.BOTH, K.narrow(recs)))
        else:
            assert runs == tg | {0} and reads == set(sorted(tg)[1::2]) | {0}, name
            at_runs |= tg
            joined += len(PR.pair(PR.PROPER, recs, 50)) if vary == "offset" else len(AR.entries(recs, 1))
    assert K.missing(at_reads, T) == [] and K.missing(at_runs, T) == [] and joined > 0


def segment_minimum(recs, a, b):
    """(where the smallest edit of records [a, b) stands, the edit) -- it stands once"""
    edits = [r[4] for r in recs[a:b]]
    assert edits.count(min(edits)) == 1
    return a + edits.index(min(edits)), min(edits)


@pytest.mark.parametrize("where", list(K.HEADLESS_AT))
def test_headless_tiles_hold_what_they_claim(where, outlier):
    T, (a, b), at = K.HEADLESS_T, K.HEADLESS_SEG, K.HEADLESS_AT[where]
    assert a // T == 0 and (b - 1) // T == 3 and at // T == {"tile1": 1, "tile2": 2, "tile0_last": 0}[where]
    assert where != "tile0_last" or at == T - 1
    headless = set(range(T, 3 * T))                                                # tiles 1 and 2
    # lca: a read
    recs, n_reads = K.headless_reads(at)
    ev = K.lca_events(recs)
    assert len(recs) == K.HEADLESS_N and (a, b) in K.reads_of(recs) and not headless & ev["heads"] and recs[-1][0] < n_reads
    (c,) = [p for p in ev["c"] if a <= p < b]
    assert at in ev["b"] and c in headless and c // T != at // T
    assert {r: t for r, t, _ in R.per_read(outlier, recs, 0)}[recs[a][0]] == recs[at][1]
    assert {r: t for r, t, _ in R.per_read(outlier, recs, ALL)}[recs[a][0]] == 100
    # abundance at the TAXID grain: a read of runs of one record
    recs, n_reads = K.headless_runs(at, "read")
    reads, runs = K.run_heads_of(recs)
    assert is_wide_list(recs, n_reads, "gi") and F.is_list(F.TAXID, K.narrow(recs)) and len(recs) == K.HEADLESS_N
    assert {a, b} <= reads and not headless & reads and runs == set(range(len(recs))) and segment_minimum(recs, a, b) == (at, 1)
    # pairs: the one run of an even read; its mate is the one record behind it
    recs, n_reads = K.headless_runs(at, "pair")
    reads, runs = K.run_heads_of(recs)
    assert is_wide_list(recs, n_reads, "offset") and len(recs) == K.HEADLESS_N
    assert {a, b, b + 1} <= reads and not headless & runs and segment_minimum(recs, a, b) == (at, 1)
    pair, mate = recs[a][0] >> 1, recs[b]
    assert recs[a][0] == 2 * pair and mate[0] == 2 * pair + 1 and {r[1:3] for r in recs[a:b + 1]} == {(5, 1)}
    assert all(abs(r[3] - mate[3]) <= 480 for r in recs[a:b])
    for mode in (PR.BOTH, PR.EITHER, PR.PROPER):
        assert (pair, 5, 1 + mate[4]) in PR.pair(mode, recs, 480, 5)
        assert (pair, 5, 3 + mate[4]) in PR.pair(mode, recs[:at] + recs[at + 1:], 480, 5)
    # abundance at the wide grains: a run inside a read that has a run before it and one behind it
    recs, n_reads = K.headless_runs(at, "abund")
    reads, runs = K.run_heads_of(recs)
    assert is_wide_list(recs, n_reads, "gi") and len(recs) == K.HEADLESS_N
    assert {30, b + 10} <= reads and not set(range(31, b + 10)) & reads and {a, b} <= runs and not headless & runs
    assert segment_minimum(recs, a, b) == (at, 2) and segment_minimum(recs, 30, b + 10) == (205, 1) and 205 // T == 3
    read, tax = recs[a][:2]
    assert AR.entries(recs, 1)[read][tax] == (1, 2) and tax not in AR.entries(recs[:at] + recs[at + 1:], 1)[read]


@pytest.mark.parametrize("T", [64, 1024])
def test_full_tiles_hold_what_they_claim(T, outlier):
    heads = K.full_tile_heads(T)
    assert set(range(T)) <= heads and T not in heads and min(h for h in heads if h >= T) == T + 9
    recs, n_reads = K.full_tile_reads(T)
    ev = K.lca_events(recs)
    assert ev["heads"] == heads and T + 3 in ev["b"] and T + 6 in ev["c"] and recs[-1][0] < n_reads
    for vary in ("offset", "gi"):
        recs, n_reads = K.full_tile_runs(T, vary)
        assert is_wide_list(recs, n_reads, vary) and K.run_heads_of(recs) == (heads, heads)
        assert segment_minimum(recs, T - 1, T + 9) == (T + 3, 1)
        assert recs[T - 1][0] % 2 == 0 and recs[T + 9][0] == recs[T - 1][0] + 1 and recs[T + 9][1] == recs[T - 1][1] == 5
    recs, n_reads = K.full_tile_runs(T, "gi", one_run=False)
    assert is_wide_list(recs, n_reads, "gi") and F.is_list(F.TAXID, K.narrow(recs))
    assert K.run_heads_of(recs) == (heads, set(range(len(recs)))) and segment_minimum(recs, T - 1, T + 9) == (T + 3, 1)


# ---- fold ----

@pytest.mark.parametrize("T", K.FOLD_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_fold_cases_hold_what_they_claim(gname, T):
    grain = GRAINS[gname]
    cases = K.fold_cases(grain, T)
    s = K.stretch(T, ceil=True)
    at_edges, better = set(), []
    for name, (a, b) in cases.items():
        assert F.is_list(grain, a) and F.is_list(grain, b), name
        which, pairs = K.fold_layout(grain, a, b)
        assert 200 <= len(which) <= max(3 * T + 50, 300), (name, len(which))
        if name.startswith("pairs"):
            tg = K.targets(T, int(name[-2:]), ceil=True)
            assert set(tg) <= set(pairs), name
            at_edges |= set(tg)
            better += [pairs[p] for p in tg]
        want = F.fold(grain, a, b)
        assert len(want) == len(which) - len(pairs) and want != a and want != b
    assert K.missing(at_edges, T, ceil=True) == []
    assert "=" not in better and abs(better.count("A") - better.count("B")) <= 3     # half of the pairs each way
    if grain == F.TAXID_GI:                                                         # ... some by the offset alone
        a, b = cases["pairs+0"]
        in_a = {F.split(grain, x)[0]: x for x in a}
        assert any(F.split(grain, y)[0] in in_a and in_a[F.split(grain, y)[0]][4] == y[4] and in_a[F.split(grain, y)[0]][3] != y[3] for y in b)
    which, pairs = K.fold_layout(grain, *cases["blocks"])
    assert which[:T] == "A" * T and which[T:2 * T] == "B" * T
    run = [p for p in sorted(pairs) if p > 2 * T]
    dense = [p for p in run if p + 2 in pairs]                                      # a dropped position at every second place
    assert len(dense) >= 2 * s and len({p // s for p in dense}) >= 3                 # ... over more than s + 1 of them, across stretch edges


# ---- text ----

@pytest.mark.parametrize("T", K.TEXT_TILES)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_text_cases_hold_what_they_claim(gname, T):
    grain = GRAINS[gname]
    cases = K.text_cases(grain, T)
    old = set(TC.cases(grain))
    assert old < set(cases)
    heads = set()
    for name, c in cases.items():
        if name in old:
            continue
        assert F.is_list(grain, c.records) and F.is_list(grain, c.second), name
        assert all(r[0] < len(c.ids) for r in c.records + c.second)
        spans, total = K.text_spans(grain, c)
        assert total == len(TC.expected(grain, c)), name                             # the spans add up to the restated text
        if name.startswith("heads"):
            d = int(name[-2:])
            tg = set(K.targets(T, d, ceil=True))
            assert tg <= K.text_heads(c) and 200 <= len(c.records) <= max(3 * T + 50, 300), name
            assert all(p + e not in K.text_heads(c) for p in tg for e in (-1, 1) if p + e > 0), name
            heads |= tg
    assert K.missing(heads, T, ceil=True) == []
    c = cases["windows"]
    spans, total = K.text_spans(grain, c)
    assert [s[0] for s in spans[::T]] + [total] == TC.tile_edges(grain, c, T)
    assert K.text_window_coverage(grain, c, T) == set(K.WINDOW_KINDS)
    want = TC.expected(grain, c)
    cap = K.text_cap(T)
    for t in range(1, len(K.WINDOW_KINDS)):                                         # read off the text itself, for the tiles of one window edge
        B = spans[t * T][0]
        W = (B & ~15) + cap
        kind = K.WINDOW_KINDS[t]
        if kind == "separator":
            assert want[W - 1:W] == b"\n"
        elif kind == "digits":
            assert want[W - 5:W + 5] == b"1234567890"
        else:
            back = {"short_id": 20, "long_id": 50}[kind]
            id_len = 2 * back
            assert want[W + back:W + back + 1] == b":" and b":" not in want[W - back:W + back] and want[W - back - 1:W - back] == b"\n"
            assert (id_len <= 64) == (kind == "short_id")
    if T == 1024:
        c = cases["residues"]
        e = TC.tile_edges(grain, c, 1024)
        assert len(e) - 1 >= 17 and {x % 16 for x in e[1:-1]} == set(range(16))


def test_big_text_equals_the_restatement_on_a_slice():
    rec, (blob, off), ids = K.big_text(n=5000)
    assert len(rec) == 5000 and len(ids) == len(off) - 1 and int(off[-1]) == len(blob)
    assert all(blob[int(off[i]):int(off[i + 1])] == s.encode() + b"\0" and 1 <= len(s) <= 3 for i, s in enumerate(ids))
    triples = list(zip(rec["read"].tolist(), rec["tax_id"].tolist(), rec["edit"].tolist()))
    assert F.is_list(F.TAXID, triples) and triples[-1][0] == len(ids) - 1
    sizes = np.bincount(rec["read"].astype(np.int64))
    assert set(sizes.tolist()) == {1, 2}
    want = K.big_text_expected(rec, ids)
    assert want == TC.text(F.TAXID, triples, ids) and want.count(b"\n") == len(ids)
    assert TC.host_format(F.TAXID, triples, (blob, off)) == want


# ---- parser ----

@pytest.mark.parametrize("T", K.PARSE_TILES)
def test_parse_texts_hold_what_they_claim(T):
    texts = K.parse_texts(T)
    s = K.stretch(T)
    starts, commas = set(), set()
    for name, lines in texts.items():
        cov = K.parse_coverage(lines)
        assert cov["bytes"] >= 3 * T, name
        assert cov["bytes"] <= 3 * max(T, 256) + 500, name
        n_reads = lines[-1][0] + 1
        for grain in K.parse_grains(name):
            recs = P.records(grain, lines, n_reads)                                # legal at the grain
            assert F.is_list(grain, recs) and len(recs) > 0
        if name.startswith("side"):
            tg = set(K.targets(T, int(name[-2:]), floor=K.PARSE_FLOOR))
            assert tg <= cov["starts"] and {p - 1 for p in tg} <= cov["commas"], name
            starts |= tg
            commas |= {p - 1 for p in tg}
    assert K.missing(starts, T, floor=K.PARSE_FLOOR) == [] and K.missing(commas, T, floor=K.PARSE_FLOOR) == []
    # the 43-byte token with 1, 21 and 42 bytes in front of a tile edge, in a run of equal keys that goes on behind the edge
    cov = K.parse_coverage(texts["straddle"])
    big = [p for p, tok in cov["tokens"] if tok == K.BIG]
    assert len(K.BIG) == 43 and sorted(-p % T for p in big) == [1, 21, 42] and all(p // T < (p + 42) // T for p in big)
    for row in cov["by_line"]:
        for (p0, t0), (p1, t1), (p2, t2) in zip(row, row[1:], row[2:]):
            if t1 == K.BIG:
                k0, k1, k2 = (P.token(t)[:2] for t in (t0, t1, t2))
                assert k0 == k1 == k2 and p0 < p1 and p1 // T < p2 // T
                assert P.token(t0)[2] < P.token(t1)[2] == P.token(t2)[2]           # LONG: the offsets ascend, then a key twice
    # lines on a tile's first byte
    cov = K.parse_coverage(texts["lines"])
    sp = K.parse_spacing(T)
    assert sp % T == 0 and {sp, 2 * sp, 3 * sp} <= cov["line_starts"]
    assert cov["empty"].get(sp, 0) == 0 and cov["empty"][2 * sp] == 1 and cov["empty"][3 * sp] == 3
    if s >= 16:                                                                     # a lane's stretch with three token starts or more
        cov = K.parse_coverage(texts["short"])
        every = cov["starts"] | cov["line_starts"]
        per_stretch = np.bincount([p // s for p in every])
        assert per_stretch.max() >= 3 and (per_stretch[:3 * T // s] >= 3).all()
    else:
        assert "short" not in texts
    lines, bad = K.parse_refused(T)
    cov = K.parse_coverage(lines)
    (p,), = [[p for p, tok in row if tok == "2-1-x=2"] for row in cov["by_line"] if any(tok == "2-1-x=2" for _, tok in row)]
    assert T - 43 <= p % T < T and p // T == 1 and cov["bytes"] >= 3 * T
    for grain in GRAINS.values():
        with pytest.raises(P.Format) as e:
            P.records(grain, lines, lines[-1][0] + 1)
        assert e.value.line == bad
