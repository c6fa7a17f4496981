"""The chain databases of helpers.chain_db are what they claim, shown with the CPU oracle alone, one read at a time: the
inputs of test_verify_rounds.py, which drives the verify rounds past the first on the device.  A read of a chain meets
its TaxID's copies in file order; every copy up to the good one is prefiltered (n_sw), the copies whose score passes
get an edit distance (n_edit), and the good copy, where there is one, is the single hit."""
import math

import numpy as np
import pytest

import helpers
from helpers import CHAIN_CASES, CHAIN_LO, CHAIN_SHAPES, chain_case, chain_prediction, expected_rounds
from oracle import oracle as O

CASE_IDS = ["%d%s" % (L, "-N" if n else "") for L, n in CHAIN_CASES]
MIN_SHARE = {False: 0.95, True: 0.90}


@pytest.mark.parametrize("L", sorted(CHAIN_SHAPES))
def test_the_copy_kinds_sit_in_their_zones(L):
    """the counts of CHAIN_SHAPES against ED = ceil(0.13 * L) and thr = L - 2 * ED, and the word counts W = 3, 5, 8"""
    sh = CHAIN_SHAPES[L]
    ED = math.ceil(L * 0.13)
    thr = L - 2 * ED
    assert sh["nG"] <= ED
    assert ED < sh["nB"] <= 2 * ED and L - 2 * sh["nB"] < thr
    assert ED < sh["s"] + sh["i"] <= 2 * ED and L - (sh["i"] + 2 * sh["s"]) >= thr
    # the read behind C's insertion: at least 20 bases, so that mismatching them is dearer than the gap
    assert L - sh["back"][1] - sh["region"] >= 20
    assert (L + 31) // 32 == {96: 3, 150: 5, 253: 8}[L]


@pytest.mark.parametrize("L,with_n", CHAIN_CASES, ids=CASE_IDS)
def test_every_seed_that_touches_the_region_is_broken_in_every_copy(L, with_n):
    """No 18-mer of a chain's segment that touches [lo, hi] occurs in a copy of it, and every copy changes lo and hi, so
    the reads keep the same intact seeds on every copy of their chain: that ties the copies in the rank order.  The
    chains are 78 (81 without N), their copies one GI each in file order under a TaxID of their own."""
    db = chain_case(L, with_n)
    region = helpers.CHAIN_N_SHAPE["region"] if with_n else CHAIN_SHAPES[L]["region"]
    lo, hi = CHAIN_LO, CHAIN_LO + region - 1
    assert len(db.chains) == (78 if with_n else 81) and len({c[0] for c in db.chains}) == len(db.chains)
    assert len(db.reads) == 6 * len(db.chains) and all(len(r) == L for r in db.reads)
    order = [e[1] for e in db.entries]
    first = 192 if with_n else lo  # (the N family: 180..191 are N in the read itself, the copies' changes start behind them)
    for (tax, kinds, gis), seg in zip(db.chains, db.segments):
        assert [order.index(g) for g in gis] == list(range(order.index(gis[0]), order.index(gis[0]) + len(gis)))
        for gi, kind in zip(gis, kinds):
            copy = db.copies[gi]
            assert copy[:lo] == seg[:lo] and copy[-(len(seg) - hi - 1):] == seg[hi + 1:], (kinds, kind)
            assert copy[first] != seg[first] and copy[-(len(seg) - hi)] != seg[hi], (kinds, kind)
            if kind in "ABG":  # as many substitutions as CHAIN_SHAPES says
                assert sum(a != b for a, b in zip(copy, seg)) == {"A": region, "B": CHAIN_SHAPES[L].get("nB"), "G": CHAIN_SHAPES[L].get("nG")}[kind]
            elif kind == "C":
                sh = CHAIN_SHAPES[L]
                assert len(copy) == len(seg) + sh["i"] and sum(a != b for a, b in zip(copy[:hi - 4], seg)) == sh["s"] - 1
            for p in range(lo - 17, hi + 1):
                if not (with_n and p < 192 and p + 18 > 180):  # (a seed that holds one of the read's N is no seed)
                    assert seg[p:p + 18] not in copy, (kinds, kind, p)
    assert sum(len(e[2]) for e in db.entries) < 1 << 18  # a test-sized database


@pytest.mark.parametrize("L,with_n", CHAIN_CASES, ids=CASE_IDS)
def test_the_oracle_walks_the_chains_as_designed(L, with_n):
    """Share of the reads whose (n_sw, n_edit, hits), binned alone at default parameters, are exactly
    helpers.chain_prediction of their chain -- (len(chain), #C + #c + #e + g, g), g = 1 when the chain ends in a good copy:
        L = 96: 486 / 486    L = 150: 486 / 486    L = 253: 468 / 486    L = 150 with N: 449 / 468
    (required: 95 %, 90 % for the N family).  The others met a copy whose inserted bases happened to align within ED, or
    picked up a further candidate; they stay in the batches of test_verify_rounds.py, where the device is compared with
    the oracle on them as on every read.  Where the chain has a good copy, the single hit is that copy's GI; the reads of
    CCCCG, CCCCCG and CCCCCCG pay 5, 6 and 7 edit distances."""
    db = chain_case(L, with_n)
    share = sum(db.as_predicted) / len(db.reads)
    print("as predicted: %d / %d" % (sum(db.as_predicted), len(db.reads)))
    assert share >= MIN_SHARE[with_n], share
    n_good = 0
    for k, ((hits, ctr), ok) in enumerate(zip(db.per_read, db.as_predicted)):
        kinds = db.kinds_of(k)
        if ok and db.good_gi(k) is not None:
            assert len(hits) == 1 and int(hits["gi"][0]) == db.good_gi(k) and int(hits["tax_id"][0]) == db.chains[db.read_chain[k]][0]
            n_good += 1
        if len(kinds) >= 5:
            assert ok and ctr["n_edit"] == len(kinds) and ctr["n_sw"] == len(kinds), (kinds, ctr)
    assert n_good >= 0.45 * len(db.reads)
    # both strands are among the predicted reads of every depth the device tests ask for
    depth = {}
    for k, ok in enumerate(db.as_predicted):
        if ok:
            depth.setdefault(expected_rounds(db.kinds_of(k)), set()).add(k % 6 < 3)
    want = (1, 2, 3) if with_n else (1, 2, 3, 4, 5, 6)
    assert sorted(depth) == list(want) and all(depth[d] == {True, False} for d in want), depth


def by_read(hits, n):
    out = [[] for _ in range(n)]
    for h in hits:
        out[int(h["read"])].append(tuple(int(h[f]) for f in helpers.FIELDS[1:]))
    return out


@pytest.mark.parametrize("L,with_n", CHAIN_CASES, ids=CASE_IDS)
def test_max_candidates_cuts_inside_the_chains(L, with_n):
    """for every max_candidates up to the longest chain less one (6; 3 in the N family) some reads lose or change their
    hit against the unlimited run and others keep it: the cut falls inside chains"""
    db = chain_case(L, with_n)
    bases, off = helpers.reads_to_batch(db.reads)
    n = len(db.reads)
    full = by_read(db.orc.bin_batch(bases, off, O.default_params(), threads=8)[0], n)
    assert full == [[tuple(int(h[f]) for f in helpers.FIELDS[1:]) for h in hits] for hits, _ in db.per_read]
    for mc in range(1, 4 if with_n else 7):
        cut = by_read(db.orc.bin_batch(bases, off, O.default_params(max_candidates=mc), threads=8)[0], n)
        differ = sum(a != b for a, b in zip(cut, full))
        assert 0 < differ < n, (mc, differ)


@pytest.mark.parametrize("kinds,rounds", [
    ("CG", 1), ("CCG", 2), ("CCCG", 3), ("CCCCG", 4), ("CCCCCG", 5), ("CCCCCCG", 6), ("CCC", 3),
    ("CBG", 2), ("BCG", 1), ("AAA", 1), ("ecg", 1), ("cecg", 2),
    ("G", 1), ("AG", 1), ("B", 1), ("BBB", 1), ("ACAG", 1), ("CAC", 2), ("CAB", 2), ("BCB", 2), ("BCCG", 2), ("CBC", 2),
    ("g", 1), ("eee", 1), ("bcg", 1), ("bec", 2), ("ccc", 3), ("cbcg", 2), ("cebg", 2), ("ebcg", 1),
])
def test_expected_rounds_on_hand_made_chains(kinds, rounds):
    """C^k G -> k, CB G -> 2, BC G -> 1, AAA -> 1, ec g -> 1, ce c g -> 2, and a few more walked by hand"""
    assert expected_rounds(kinds) == rounds


def test_chain_prediction_counts():
    assert chain_prediction("ABCG") == (4, 2, 1) and chain_prediction("CCC") == (3, 3, 0) and chain_prediction("A") == (1, 0, 0)
    assert chain_prediction("ebcg") == (4, 3, 1) and chain_prediction("bb") == (2, 0, 0)
    assert np.all([chain_prediction(k)[0] == len(k) for k in helpers.chain_kinds() + helpers.chain_kinds(True)])
