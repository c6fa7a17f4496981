"""-m gpu: long merged windows of non-repeating text at the edges of the verify kernels' window stores.

Every verify kernel holds a part of a candidate window at a time: k_sw_pairs a ring of 512 columns per candidate, refilled
256 columns at a time, k_evaluate (reads of 254 bases and more, and MTSV_SW=packed) a ring of 1 024 columns refilled by
halves, k_edit_myers two 64-byte sectors of a stream that a quad of lanes fetches together.  A window outgrows these stores
only where seed hits merge, and on a tandem repeat a stale, shifted or missing refill leaves copies of the same unit in the
store: the read finds its alignment, with the same score and distance, in another copy.  The windows of window_cases.py
are random text, as long as planned to the column, with the read's true alignment at a planned place in them
(test_long_windows_cpu.py holds the cases to that by the oracle alone).

Every batch is compared hit for hit, all six fields, with the CPU oracle, and the counters n_seed_hits, n_candidates,
n_verified, window_bytes with the oracle's; in the reference order of reads up to 253 bases n_sw_passed is the oracle's
n_edit as well (no read here holds an N)."""
import os
import random

import pytest

import helpers
import mtsv_tools_amd as M
import window_cases as wc
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VS_ORACLE = ("n_seed_hits", "n_candidates", "n_verified", "window_bytes")
VS_LEGACY = VS_ORACLE + ("n_hits", "n_sw_passed", "n_sw_bound_refuted", "n_rounds", "myers_columns")
# the verify arrangements of reads up to 253 bases: the switches a workspace reads when it is created
ARRANGEMENTS = {
    "fused": {},                                   # k_edit_myers fused, k_sw_pairs, k_edit_myers list mode
    "legacy": {"MTSV_MYERS_FETCH": "legacy"},      # every lane of k_edit_myers fetches its own window
    "bound+list": {"MTSV_SW_FUSED": "0"},          # k_sw_diag, k_edit_myers as the bound, k_sw_pairs, list mode
    "chain": {"MTSV_VERIFY": "edit_first"},        # k_edit_myers alone, walking the chains itself
    "packed": {"MTSV_SW": "packed"},               # the register k_evaluate<R>, ring 1 024
}
COUNTS_PASSED = ("fused", "legacy", "bound+list")  # (n_sw_passed is kept by the reference order in rounds)
SWITCHES = sorted({k for env in ARRANGEMENTS.values() for k in env})


class Db:
    def __init__(self, tmp):
        d = wc.database()
        self.ix = M.MGIndex.build(d.entries, threads=4)
        path = str(tmp / "windows.idx")
        self.ix.write(path)
        self.orc = O.Index.read(path)
        self.ix.to_device(0)
        self.wanted = {}

    def oracle(self, key, reads, rate):
        """the oracle's (hits, counters) of a batch, computed once per key and left unchanged"""
        if key not in self.wanted:
            bases, off = helpers.reads_to_batch(reads)
            self.wanted[key] = self.orc.bin_batch(bases, off, O.default_params(edit_rate=rate, **wc.SEED), threads=8)
        return self.wanted[key]


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    d = Db(tmp_path_factory.mktemp("windows"))
    yield d
    d.ix.close()


def workspace(ix, arrangement, n_reads, n_bases):
    assert not any(k in os.environ for k in SWITCHES)
    env = ARRANGEMENTS[arrangement]
    try:
        os.environ.update(env)
        return M.Batch(ix, 0, n_reads, n_bases)
    finally:
        for k in env:
            os.environ.pop(k, None)


def run(db, key, reads, rate, arrangement="fused", min_hits=0):
    """one batch in one arrangement against the oracle; returns the workspace's stats"""
    bases, off = helpers.reads_to_batch(reads)
    want, ctr = db.oracle(key, reads, rate)
    assert len(want) >= min_hits, (len(want), min_hits)
    b = workspace(db.ix, arrangement, len(reads), len(bases))
    try:
        b.upload(bases, off)
        b.run(M.default_params(edit_rate=rate, **wc.SEED))
        got, st = b.download(), b.stats()
    finally:
        b.close()
    assert_same_hits(got, want)
    assert tuple(st[k] for k in VS_ORACLE) + (st["n_hits"],) == (ctr["H"], ctr["n_cand"], ctr["n_sw"], ctr["W"], len(want)), arrangement
    if arrangement in COUNTS_PASSED and max(map(len, reads)) <= 253:
        assert st["n_sw_passed"] == ctr["n_edit"], arrangement
    return st


def min_hits_of(group):
    return sum(3 * r.n // 4 for r in wc.GROUPS[group] if r.must_hit)


# ---- 1. reads up to 253 bases: the pairs ring, the sector stream, the register k_evaluate ----------------------------------
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("group", wc.PAIRS_GROUPS)
def test_windows_at_the_edges_of_the_pairs_ring(db, group, arrangement):
    """windows of 511 .. 1 025 columns and of 2 021, the body at the end, at the start and in the middle of each, both
    strands, for reads of 96, 150 and 253 bases; the body across columns 512 and 768 from either end, runs of N across
    them, and windows clipped at the first and the last symbol of the text.  The groups whose names end in "u" hold the same
    windows with a read that the bound of k_edit_myers leaves undecided (window_cases.undecided_gap): in the reference order
    only these reach the sweep of k_sw_pairs, whose verdict shows in n_sw_passed.  "legacy" runs the default workspace as well:
    what the oracle does not count is equal between the two."""
    reads = [rd.seq for rd in wc.group_reads(group)]
    st = run(db, group, reads, wc.group_rate(group), arrangement, min_hits_of(group))
    if group.endswith("u") and arrangement in COUNTS_PASSED:  # the bound leaves these to the sweep of k_sw_pairs
        assert st["sw_cell_pairs"] > 0 and st["n_sw_passed"] >= len(reads) > 4 * st["n_hits"]
    if arrangement == "legacy":
        new = run(db, group, reads, wc.group_rate(group), "fused")
        assert [new[k] for k in VS_LEGACY] == [st[k] for k in VS_LEGACY], [(k, new[k], st[k]) for k in VS_LEGACY]
        assert st["myers_columns"] > 0


# ---- 2. reads of 254 bases and more: k_evaluate's ring in the register word kernel and in the tiled kernel ------------------
@pytest.mark.parametrize("group", wc.EVAL_GROUPS)
def test_windows_at_the_edges_of_the_evaluate_ring(db, group):
    """windows of 1 023 .. 2 049 columns, of 4 200 and of 10 073; 254 and 256 bases run the register word kernel, 257, 300,
    600 and 1 000 the tiled kernel, whose strip is as long as the longest window of the pass; the body across columns
    1 024 and 1 536, runs of N across them, clipped windows"""
    reads = [rd.seq for rd in wc.group_reads(group)]
    run(db, group, reads, wc.group_rate(group), min_hits=min_hits_of(group))


# ---- 3. neighbours ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_one_long_window_beside_three_short_ones(db, arrangement):
    """at the default rate one read in four has a window of 511 .. 1 273 columns, the others windows of w columns, a part of
    them refuted with successors to walk on to: a quad of k_edit_myers holds one long window beside three short ones, a pair
    of k_sw_pairs a long half and a short half"""
    st = run(db, "neighbours", wc.neighbours_batch(), 0.13, arrangement, min_hits=100)
    if arrangement == "fused":
        assert st["sw_cell_pairs"] > 0


def mixed_lengths():
    """every third read of the 253-base and the 150-base groups at rate 0.3, shuffled: only long windows, 511 .. 2 021
    columns, of two read lengths, decided by the bound or left to the sweep"""
    reads = [rd.seq for g in ("p253b", "p253bu", "p-edges", "p-edges-u", "p150", "p150u", "p150-edges") for rd in wc.group_reads(g)[::3]]
    random.Random(0x3153).shuffle(reads)
    return reads


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_only_long_windows_of_different_lengths(db, arrangement):
    reads = mixed_lengths()
    run(db, "mixed", reads, 0.3, arrangement, min_hits=len(reads) // 2)


@pytest.mark.parametrize("group,k", [("p150", 73), ("p253b", 232), ("p253b", 233), ("e256", 100), ("e300", 101)])
def test_a_single_read(db, group, k):
    """count = 1: one long window alone in its quad, its pair and its wavefront (p253b 232 / 233: 2 021 columns, either
    strand)"""
    rd = wc.group_reads(group)[k]
    assert rd.window[1] - rd.window[0] > (wc.RING_PAIRS if group[0] == "p" else wc.RING_EVAL)
    for arrangement in (ARRANGEMENTS if group[0] == "p" else ("fused",)):
        st = run(db, (group, k), [rd.seq], wc.group_rate(group), arrangement)
        assert (st["n_candidates"], st["n_hits"]) == (1, 1)


# ---- 4. all three outcomes of the two checks on long windows, at the default rate ---------------------------------------
@pytest.mark.parametrize("arrangement", ("fused", "bound+list"))
def test_substituted_bodies_refuted_refused_and_accepted(db, arrangement):
    """0 .. 9 substitutions in the first 60 bases of the body: windows of 568, 1 027 and 1 273 columns that the prefilter
    refutes, that pass it and are refused by the edit distance, and that hit"""
    reads = [rd.seq for r in wc.SUBS_RUNGS for rd in r.reads()]
    st = run(db, "subs", reads, 0.13, arrangement, min_hits=15)
    want, ctr = db.oracle("subs", reads, 0.13)
    assert ctr["n_sw"] - ctr["n_edit"] >= 15 and ctr["n_edit"] - len(want) >= 15
    assert st["n_sw_passed"] == ctr["n_edit"] and st["sw_cell_pairs"] > 0
