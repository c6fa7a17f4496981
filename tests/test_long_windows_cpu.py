"""The cases of window_cases.py are what they claim, by the CPU oracle alone: every read of every rung forms exactly one
candidate, its window has the planned length (the clipped length, where the rung is cut at its bin), the rungs that are
meant to hit do, the rungs meant for the sweep pass the score and are refused by the edit distance, and the rungs with
substitutions in the body hold all three outcomes of the reference's two checks (index.rs:406 / :410).  A change of a generator cannot empty test_long_windows.py unnoticed."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import helpers
import window_cases as wc
from oracle import oracle as O


@pytest.fixture(scope="module")
def orc():
    return O.Index.build(wc.database().entries)


def per_read(orc, reads, rate):
    """[(hits, counters)] of every read binned alone"""
    op = O.default_params(edit_rate=rate, **wc.SEED)

    def one(rd):
        b, o = helpers.reads_to_batch([rd if isinstance(rd, bytes) else rd.seq])
        return orc.bin_batch(b, o, op, threads=1)

    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, reads))


def planned_window(rung, rd):
    """(start, end) of the union of the windows of the read's planned seed hits, each cut at its bin as the reference does"""
    d = wc.database()
    lo, hi = d.bin_of("main" if rung.where == "main" else rung.where)
    spans = [O.candidate_indices(site, q, lo, hi, rung.L, rung.ED) for site, q in rd.sites]
    assert all(spans)
    return min(s for s, _ in spans), max(e for _, e in spans)


def check_rung(orc, rung):
    reads = rung.reads()
    assert len(reads) == rung.n and {rd.strand for rd in reads} == {0, 1}
    res = per_read(orc, reads, rung.rate)
    lo, hi = wc.database().bin_of("main" if rung.where == "main" else rung.where)
    for rd, (hits, c) in zip(reads, res):
        assert b"N" not in rd.seq
        s, e = planned_window(rung, rd)
        assert (c["n_cand"], c["n_sw"], c["W"]) == (1, 1, e - s), (rung, rd.P, c, e - s)
        if rung.where == "first":
            assert s == lo and rung.W - rung.ED <= e - s < rung.W
        elif rung.where == "last":
            assert e == hi and rung.W - rung.ED <= e - s < rung.W
        else:
            assert (s, e) == rd.window and e - s == rung.W
        assert all(int(h["strand"]) == rd.strand and int(h["offset"]) == s - lo for h in hits)
    if rung.clipped:
        assert len({c["W"] for _, c in res}) >= rung.n - 1  # (a column more or less from read to read)
    return res


@pytest.mark.parametrize("group", list(wc.GROUPS))
def test_every_read_forms_one_window_of_the_planned_length(orc, group):
    for rung in wc.GROUPS[group]:
        res = check_rung(orc, rung)
        n_hit = sum(len(h) == 1 for h, _ in res)
        if rung.must_hit:
            assert 4 * n_hit >= 3 * rung.n, (rung, n_hit)
        if rung.gap:  # meant for the sweep: the score passes every read, the edit distance refuses three quarters at least
            assert all(c["n_edit"] == 1 for _, c in res) and 4 * n_hit <= rung.n, (rung, n_hit)


def test_window_lengths_sit_on_both_sides_of_every_ring_edge():
    """what the groups hold: the lengths around one, one and a half and two rings for every kernel, the body at the end, at
    the start and in the middle of each, a window of 2 000 columns or more for the pairs ring and one beyond four rings of
    k_evaluate, the body across every refill boundary, an N run across each, and windows cut at both ends of a bin"""
    for g, ring, lengths in (("p150", 512, wc.PAIRS_LENGTHS), ("p253a", 512, wc.PAIRS_LENGTHS), ("p253b", 512, wc.PAIRS_LENGTHS + (2021,)),
                             ("p253bu", 512, wc.PAIRS_LENGTHS + (2021,)),
                             ("e254", 1024, wc.EVAL_LENGTHS), ("e256", 1024, wc.EVAL_LENGTHS), ("e257", 1024, wc.EVAL_LENGTHS),
                             ("e300", 1024, wc.EVAL_LENGTHS), ("e600", 1024, wc.EVAL_LENGTHS + (4200,))):
        assert set(lengths) >= {ring * k // 2 + d for k in (2, 3, 4) for d in (-1, 0, 1)}
        for W in lengths:
            rungs = [r for r in wc.GROUPS[g] if r.W == W]
            assert len(rungs) == 3
            assert sorted((bool(r.head), bool(r.tail)) for r in rungs) == [(False, True), (True, False), (True, True)]
    assert {r.W for r in wc.GROUPS["p96"]} == {460, 511, 512, 513}
    assert max(r.W for r in wc.GROUPS["e600"]) > 4 * wc.RING_EVAL and wc.GROUPS["e1000"][0].W == 10073
    for g, cols in (("p-edges", (512, 768)), ("e300-edges", (1024, 1536)), ("e256-edges", (1024,))):
        for col in cols:
            across = [r for r in wc.GROUPS[g] if r.name.endswith("-across%d" % col)]
            assert len(across) == 1 and across[0].head and across[0].tail
            assert 40 <= col - across[0].body_col <= 100 and across[0].body_col + across[0].L > col
            back = across[0].W - across[0].body_col - across[0].L  # the same from the window's end, for the backward walk
            assert 40 <= col - back <= 100
    for g, cols in (("p-edges", (512, 768)), ("p-edges-u", (512, 768)), ("p150-edges", (512,)), ("e300-edges", (1024, 1536))):
        assert {(r.n_col, r.n_from_end) for r in wc.GROUPS[g] if r.where == "n"} == {(c, e) for c in cols for e in (False, True)}
        assert {r.where for r in wc.GROUPS[g]} >= {"first", "last", "n"}
    for g in wc.PAIRS_GROUPS:
        assert all(r.L <= 253 and bool(r.gap) == g.endswith("u") for r in wc.GROUPS[g])
    for g in wc.EVAL_GROUPS:
        assert all(r.L >= 254 for r in wc.GROUPS[g])


def test_n_runs_lie_across_the_refill_boundaries():
    d = wc.database()
    for g in ("p-edges", "p-edges-u", "p150-edges", "e300-edges"):
        for rung in wc.GROUPS[g]:
            if rung.where != "n":
                continue
            seen = set()
            for rd in rung.reads():
                s, e = rd.window
                cols = [i - s for i in range(s, e) if d.text[i] == 78]
                assert cols and cols == list(range(cols[0], cols[0] + len(cols)))  # one run in the window
                edge = rung.W - rung.n_col if rung.n_from_end else rung.n_col
                assert cols[0] < edge <= cols[-1], (rung, cols, edge)  # N on both sides of the boundary
                seen.add((len(cols), rd.strand))
            assert seen == {(run, st) for run in wc.N_RUNS for st in (0, 1)}


def test_the_last_sequence_ends_the_text():
    d = wc.database()
    assert d.bin_of("first")[0] == 0 and d.bin_of("last")[1] == d.n - 1 == len(d.text)
    assert 20_000 <= d.n <= 60_000
    assert len({e[0] for e in d.entries}) >= 5


@pytest.mark.parametrize("rung", wc.SUBS_RUNGS, ids=repr)
def test_substituted_bodies_hold_all_three_outcomes(orc, rung):
    res = check_rung(orc, rung)
    refuted = sum(c["n_edit"] == 0 for _, c in res)
    edit_refused = sum(c["n_edit"] == 1 and len(h) == 0 for h, c in res)
    hit = sum(len(h) == 1 for h, _ in res)
    assert refuted + edit_refused + hit == rung.n
    assert min(refuted, edit_refused, hit) >= 5, (rung, refuted, edit_refused, hit)


def test_neighbours_batch_has_one_long_window_in_four(orc):
    reads = wc.neighbours_batch()
    long_seqs = {rd.seq for r in wc.GROUPS["p253a"] + wc.GROUPS["p253au"] for rd in r.reads()} | {rd.seq for rd in wc.SUBS_RUNGS[1].reads()}
    is_long = [r in long_seqs for r in reads]
    n_long = sum(is_long)
    assert n_long >= 60
    for q in range(n_long):  # one in every aligned four, at every place of the four
        assert sum(is_long[4 * q:4 * q + 4]) == 1
    assert {is_long[4 * q:4 * q + 4].index(True) for q in range(n_long)} == {0, 1, 2, 3}
    op = O.default_params(**wc.SEED)
    b, o = helpers.reads_to_batch(reads)
    want, ctr = orc.bin_batch(b, o, op, threads=8)
    short_hit = {int(r) for r in want["read"] if not is_long[int(r)]}
    n_short = len(reads) - n_long
    assert 0 < len(short_hit) < n_short - 20       # ordinary reads that hit, and at least 20 that are refused
    d = wc.database()
    for L in wc.CHAINS:  # the chains: reads whose first window is refused and that go on to a successor
        walked = [c["n_sw"] for _, c in per_read(orc, d.chain_reads[L], 0.13)]
        assert sum(n >= 2 for n in walked) >= len(walked) // 2 and max(walked) >= 3, (L, walked)
