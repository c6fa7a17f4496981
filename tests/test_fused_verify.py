"""-m gpu: the fused verify pass.  In the reference order, for reads of up to 253 bases, round 0 of a pass is one launch of
k_edit_myers in fused mode over the whole worklist: the unit-cost distance D under the SW matrix's matches refutes the
prefilter of index.rs:406 (D > 2*ED), passes it (D <= ED) and -- when the read holds no N or the window holds none -- is the
edit distance of :407-410 itself; a read N facing a window N sends the lane through a second pass under the edit
distance's matches; ED < D <= 2*ED goes to the sweep (k_sw_pairs) and from there to list mode.  MTSV_SW_FUSED=0 keeps the
arrangement before it (k_sw_diag -> bound mode -> k_sw_pairs -> list mode), MTSV_SW_BOUND=0 the one without a Myers bound.
Every batch is compared hit for hit with the CPU oracle and its counters with the oracle's."""
import math
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("n_candidates", "n_verified", "window_bytes", "n_sw_passed", "n_hits")


def both_params(**over):
    mp = M.default_params(**{("seed_interval" if k == "seed_gap" else k): v for k, v in over.items()})
    op = O.default_params(**{("seed_gap" if k == "seed_interval" else k): v for k, v in over.items()})
    return mp, op


def make_batch(ix, n_reads, n_bases, monkeypatch, fused=None, bound=None, **kw):
    """a workspace; the switches are read when it is created"""
    for name, v in (("MTSV_SW_FUSED", fused), ("MTSV_SW_BOUND", bound)):
        if v is not None:
            monkeypatch.setenv(name, v)
    try:
        return M.Batch(ix, 0, n_reads, n_bases, **kw)
    finally:
        monkeypatch.delenv("MTSV_SW_FUSED", raising=False)
        monkeypatch.delenv("MTSV_SW_BOUND", raising=False)


def run_resident(ix, bases, off, mp, monkeypatch, fused=None, bound=None):
    b = make_batch(ix, len(off) - 1, len(bases), monkeypatch, fused, bound)
    b.upload(bases, off)
    b.run(mp)
    got, st = b.download(), b.stats()
    b.close()
    return got, st


def check(got, st, want, ctr, what=None):
    assert_same_hits(got, want)
    assert tuple(st[k] for k in COUNTERS) == (ctr["n_cand"], ctr["n_sw"], ctr["W"], ctr["n_edit"], len(want)), what


def index_of(entries, tmp_path, name):
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path / f"{name}.idx")
    ix.write(p)
    ix.to_device(0)
    return ix, O.Index.read(p)


def n_count(r):
    return sum(c not in b"ACGTacgt" for c in r)


def few_n(reads, edit_rate=0.13):
    """reads with at most ED positions that are no base: a read with more can have no hit, its strands never reach the
    verify kernels and the device does not count what the prefilter would have passed for them"""
    return [r for r in reads if n_count(r) <= math.ceil(len(r) * edit_rate)]


def edited(rng, src, n_sub, n_del, n_ins):
    """src with n_del bases left out, n_ins put in and n_sub substituted, at random places"""
    s = bytearray(src)
    for _ in range(n_del):
        del s[rng.randrange(5, len(s) - 5)]
    for _ in range(n_ins):
        s.insert(rng.randrange(5, len(s) - 5), rng.choice(b"ACGT"))
    return helpers.substitute(rng, bytes(s), n_sub)


def d_sw(read, win):
    """the unit-cost semi-global distance under the SW matrix's matches (N matches N)"""
    w = np.frombuffer(win, dtype=np.uint8)
    idx = np.arange(len(w) + 1)
    prev = np.zeros(len(w) + 1, dtype=np.int64)
    for i, r in enumerate(read, 1):
        tmp = np.empty(len(w) + 1, dtype=np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(prev[:-1] + (w != r), prev[1:] + 1)
        prev = np.minimum.accumulate(tmp - idx) + idx
    return int(prev.min())


def n_run_db(rng):
    """six sequences of 9000 bases; the last holds N runs of 1..30 bases, 280 bases apart.  Returns (entries, [(start, k)])"""
    entries = [(10 + t, 500 + t, helpers.rnd_seq(rng, 9000)) for t in range(6)]
    body = bytearray(entries[5][2])
    runs = []
    for k in range(1, 31):
        at = 300 + 280 * (k - 1)
        body[at:at + k] = b"N" * k
        runs.append((at, k))
    entries[5] = (15, 505, bytes(body))
    return entries, runs


# ---- 1. the three arrangements decide alike --------------------------------------------------------------------------
def test_fused_default_equals_the_two_older_arrangements(tmp_path, monkeypatch):
    """one mixed batch -- the adversarial database's reads (conserved gene, tandem repeat, N, junk bytes, clipped windows)
    and the bound test's classes (indels, D in every zone) -- in the fused arrangement (the default), with MTSV_SW_FUSED=0
    and with MTSV_SW_BOUND=0: the oracle's hits and counters three times, and the stage timers say which kernels ran"""
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix, orc = index_of(entries, tmp_path, "mixed")
    reads = [r for r in helpers.tricky_reads(entries, gene, unit, seed=12, n_each=40, lengths=(100, 150, 253)) if len(r) <= 253]
    rng = random.Random(5)
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    for i in range(300):
        t = rng.choice(texts)
        st = rng.randrange(0, len(t) - 170)
        kind = i % 4
        if kind == 0:
            r = edited(rng, t[st:st + 154], 3, 4, 2)[:150]
        elif kind == 1:
            r = edited(rng, t[st:st + 164], 8, 14, 0)[:150]
        elif kind == 2:
            r = helpers.substitute(rng, t[st:st + 150], 26)
        else:
            r = bytearray(helpers.rnd_seq(rng, 150))
            at = rng.randrange(0, 8) * 15
            r[at:at + 18] = t[st:st + 18]
            r = bytes(r)
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    reads = few_n(reads)
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params()
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    assert len(want) > 300 and ctr["n_edit"] > len(want)
    stats = {}
    for name, fused, bound in (("fused", None, None), ("unfused", "0", None), ("no_bound", None, "0")):
        got, st = run_resident(ix, bases, off, mp, monkeypatch, fused, bound)
        check(got, st, want, ctr, name)
        stats[name] = st
    assert stats["fused"]["sw_diag_ms"] == 0 and stats["fused"]["sw_bound_ms"] > 0 and stats["fused"]["n_sw_bound_refuted"] > 0
    assert stats["unfused"]["sw_diag_ms"] > 0 and stats["unfused"]["sw_bound_ms"] > 0 and stats["unfused"]["n_sw_bound_refuted"] > 0
    assert stats["no_bound"]["sw_diag_ms"] > 0 and stats["no_bound"]["sw_bound_ms"] == 0 and stats["no_bound"]["n_sw_bound_refuted"] == 0
    # the fused pass advances the columns of every candidate once; the sweep sees only what lies between its thresholds
    assert 0 < stats["fused"]["sw_cell_pairs"] < stats["no_bound"]["sw_cell_pairs"]
    assert stats["fused"]["myers_columns"] > 0


# ---- 2. N facing N: the second pass ----------------------------------------------------------------------------------
def test_read_n_facing_window_n_takes_the_second_pass(tmp_path, monkeypatch):
    """Reads cut across the N runs of a database sequence: their k N face the window's k N, a match in the SW matrix and
    a mismatch in the edit distance, so D(SW) = the other substitutions s and the edit distance = s + k.  s = 0, ED - k,
    ED, ED + 1: accepted with an `edit` above D(SW) (the single-pass shortcut would report D), passed by index.rs:406
    and refused by :410 (s = ED), left to the sweep and refuted (s = ED + 1).  Both strands."""
    rng = random.Random(31)
    entries, runs = n_run_db(rng)
    ix, orc = index_of(entries, tmp_path, "nruns")
    L = 150
    ED = math.ceil(L * 0.13)
    text = entries[5][2]
    reads, origin = [], []
    for at, k in runs:
        if k > ED:
            continue
        for s in (0, max(ED - k, 0), ED, ED + 1):
            for _ in range(3):
                st = rng.randrange(at + k + 12 - L, at - 12)
                r = bytearray(text[st:st + L])
                free = [i for i in range(L) if r[i] != ord("N")]
                for i in rng.sample(free, s):
                    r[i] = rng.choice([c for c in b"ACGT" if c != r[i]])
                r = bytes(r)
                assert n_count(r) == k
                origin.append((r, text[st - ED:st + L + ED]))
                reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    # with the oracle alone: enough reads of both kinds that tell the second pass from the shortcut
    refused = accepted_above = 0
    for r, win in origin:
        edits = O.min_edit_distance(r.replace(b"N", b"."), win)
        if O.ssw_score(r, win) >= L - 2 * ED and edits > ED and d_sw(r, win) <= ED:
            refused += 1
        if edits <= ED and d_sw(r, win) < edits:
            accepted_above += 1
    assert refused >= 20 and accepted_above >= 20, (refused, accepted_above)
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params()
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    found = set(want["read"].tolist())  # (a read so damaged that no seed of it is left intact is never verified)
    assert sum(1 for i, (r, win) in enumerate(origin) if i in found and d_sw(r, win) < O.min_edit_distance(r.replace(b"N", b"."), win)) >= 20
    assert ctr["n_edit"] >= len(want) + 20
    for fused in (None, "0"):
        got, st = run_resident(ix, bases, off, mp, monkeypatch, fused)
        check(got, st, want, ctr, fused)
        assert st["n_sw_passed"] > st["n_hits"]  # passed index.rs:406, refused by :410
    # runs longer than ED: the read holds more N than edits are allowed, its strands are dropped before the verify stage
    hopeless = []
    for at, k in runs:
        if k > ED:
            st = rng.randrange(at + k + 12 - L, at - 12)
            r = text[st:st + L]
            hopeless += [r, helpers.revcomp(r)]
    hb, ho = helpers.reads_to_batch(reads[:40] + hopeless)
    hwant, hctr = orc.bin_batch(hb, ho, op, threads=8)
    got, st = run_resident(ix, hb, ho, mp, monkeypatch)
    assert_same_hits(got, hwant)
    assert (st["n_candidates"], st["n_verified"], st["window_bytes"]) == (hctr["n_cand"], hctr["n_sw"], hctr["W"])


# ---- 3. N on one side only: the single-pass shortcut -----------------------------------------------------------------
def test_n_on_one_side_only_is_decided_in_one_pass(tmp_path, monkeypatch):
    """reads with N against windows without, and reads without N against windows with N runs (the run's bases replaced
    in the read): no N faces an N, D is the edit distance, and every accepted candidate reports it"""
    rng = random.Random(32)
    entries, runs = n_run_db(rng)
    ix, orc = index_of(entries, tmp_path, "oneside")
    L = 150
    ED = math.ceil(L * 0.13)
    text = entries[5][2]
    reads = []
    for i in range(240):  # N in the read, none in the window
        t = entries[rng.randrange(5)][2]
        st = rng.randrange(0, len(t) - L - 10)
        r = helpers.substitute(rng, t[st:st + L], rng.randrange(1, ED + 1), alpha=b"N")
        r = helpers.substitute(rng, r, rng.choice([0, 2, ED - n_count(r), ED + 1 - n_count(r)]), alpha=b"ACGT")
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    for at, k in runs:  # N in the window, none in the read
        for s in (0, max(ED - k, 0), max(ED + 1 - k, 0)):
            for _ in range(2):
                st = rng.randrange(at + k + 12 - L, at - 12)
                r = bytes(c if c != ord("N") else rng.choice(b"ACGT") for c in text[st:st + L])
                r = helpers.substitute(rng, r, s)
                reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    reads = few_n(reads)
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params()
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    assert len(want) > 150 and 0 < len(set(want["read"].tolist())) < len(reads)
    for fused in (None, "0"):
        got, st = run_resident(ix, bases, off, mp, monkeypatch, fused)
        check(got, st, want, ctr, fused)


# ---- 4. the undecided zone -------------------------------------------------------------------------------------------
def test_between_the_thresholds_the_sweep_decides_in_the_same_round(tmp_path, monkeypatch):
    """ED < D <= 2*ED for the read's origin: 14 bases of the reference left out + 8 substitutions (score passes, the
    edit distance refuses), 26 substitutions (the sweep refutes), 10 left out + 2 substitutions + an insertion (D = 13,
    decided by the fused pass alone)"""
    rng = random.Random(33)
    entries = [(10 + t, 500 + t, helpers.rnd_seq(rng, 6000)) for t in range(6)]
    ix, orc = index_of(entries, tmp_path, "undecided")
    L = 150
    reads = []
    for i in range(300):
        t = entries[rng.randrange(6)][2]
        st = rng.randrange(0, len(t) - L - 40)
        kind = i % 3
        if kind == 0:
            r = edited(rng, t[st:st + L + 14], 8, 14, 0)[:L]
        elif kind == 1:
            r = helpers.substitute(rng, t[st:st + L], 26)
        else:
            r = edited(rng, t[st:st + L + 9], 2, 10, 1)[:L]
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params()
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    assert len(want) > 60 and ctr["n_edit"] >= len(want) + 40
    got, st = run_resident(ix, bases, off, mp, monkeypatch)
    check(got, st, want, ctr)
    assert st["sw_cell_pairs"] > 0 and st["sw_diag_ms"] == 0
    assert st["n_rounds"] == 1  # the sweep ran in the round of the fused pass
    got0, st0 = run_resident(ix, bases, off, mp, monkeypatch, fused="0")
    check(got0, st0, want, ctr)


# ---- 5. chains of one TaxId ------------------------------------------------------------------------------------------
def test_successors_of_a_failed_candidate_are_decided_in_the_fused_pass(tmp_path, monkeypatch):
    """Two copies of a segment under one TaxId with the same seeds knocked out, so that they tie in the rank order, in both
    database orders (two TaxIds): a damaged copy (60 bases changed: refuted; or an N run facing the read's N plus 17
    substitutions: passed by index.rs:406, refused by :410) and the good copy that is the hit.  The oracle, one read at a
    time, shows that chains were walked.  Then the conserved gene of the adversarial database, with max_candidates
    cutting the chains."""
    rng = random.Random(34)
    L = 150
    seg_a, seg_b = helpers.rnd_seq(rng, 400), helpers.rnd_seq(rng, 400)

    def changed(seg, positions):
        s = bytearray(seg)
        for i in positions:
            s[i] = helpers.COMP[s[i]]
        return s

    # every 18-mer that touches 180..269 holds a changed base in both copies: a read of seg_a loses the same seeds on both
    refuted_copy = bytes(changed(seg_a, range(180, 270)))                        # 90 substitutions: D > 2*ED
    good_copy = bytes(changed(seg_a, list(range(180, 270, 12)) + [269]))         # 9
    # the reads of seg_b hold N at 180..191; every 18-mer that touches 180..209 holds an N or the changed base 209
    refused_copy = changed(seg_b, range(192, 210))                               # N faces N, 18 substitutions (a gapped alignment
    refused_copy[180:192] = b"N" * 12                                            # does with ~13): D(SW) <= ED < D(SW) + 12 = edits
    refused_copy = bytes(refused_copy)
    plain_copy = bytes(changed(seg_b, [209]))                                    # bases under the read's N: 13 edits

    def flank(s):
        return helpers.rnd_seq(rng, rng.randrange(80, 200)) + s + helpers.rnd_seq(rng, rng.randrange(80, 200))

    entries = [(10 + t, 500 + t, helpers.rnd_seq(rng, 4000)) for t in range(4)]
    entries += [(70, 701, flank(refuted_copy)), (70, 702, flank(good_copy)),
                (71, 711, flank(good_copy)), (71, 712, flank(refuted_copy)),
                (72, 721, flank(refused_copy)), (72, 722, flank(plain_copy)),
                (73, 731, flank(plain_copy)), (73, 732, flank(refused_copy))]
    ix, orc = index_of(entries, tmp_path, "chains")
    src_b = bytearray(seg_b)
    src_b[180:192] = b"N" * 12
    src_b = bytes(src_b)
    reads = []
    for i in range(200):
        st = rng.randrange(120, 170)
        src = seg_a if i % 2 == 0 else src_b
        r = helpers.substitute(rng, src[st:st + L], rng.randrange(0, 4), lo=0, hi=10)
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    mp, op = both_params()

    def one(r):
        b, o = helpers.reads_to_batch([r])
        return orc.bin_batch(b, o, op, threads=1)

    with ThreadPoolExecutor(8) as ex:
        per_read = list(ex.map(one, reads))
    # A read has two candidates under each of two TaxIds, and a TaxId is left once a candidate of it is a hit: a third
    # prefilter run (a third edit distance) beside the two hits means that a damaged copy came first and its chain was walked.
    walked_refuted = sum(1 for (h, c), r in zip(per_read, reads) if n_count(r) == 0 and len(h) == 2 and c["n_sw"] >= 3)
    walked_refused = sum(1 for (h, c), r in zip(per_read, reads) if n_count(r) and len(h) == 2 and c["n_edit"] >= 3)
    assert walked_refuted >= 20 and walked_refused >= 20, (walked_refuted, walked_refused)
    bases, off = helpers.reads_to_batch(reads)
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    for fused in (None, "0"):
        got, st = run_resident(ix, bases, off, mp, monkeypatch, fused)
        check(got, st, want, ctr, fused)
        assert st["n_rounds"] == 1 or fused == "0"  # every successor inside the fused pass: no further round
    # the conserved gene: up to 24 candidates of 8 TaxIds per read, chains cut by max_candidates
    tentries, gene, unit = helpers.tricky_db(seed=7)
    tix, torc = index_of(tentries, tmp_path, "gene")
    treads = few_n([r for r in helpers.tricky_reads(tentries, gene, unit, seed=13, n_each=60, lengths=(150, 100)) if len(r) <= 253])
    tb, to = helpers.reads_to_batch(treads)
    for mc in (-1, 6, 3, 1):
        mp, op = both_params(max_candidates=mc)
        want, ctr = torc.bin_batch(tb, to, op, threads=8)
        assert len(want) > 50
        got, st = run_resident(tix, tb, to, mp, monkeypatch)
        check(got, st, want, ctr, mc)


# ---- 6. tolerances, read lengths, the host path ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder_db(tmp_path_factory):
    entries, _, _ = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "fused_ladder.idx")
    ix.write(p)
    return ix, O.Index.read(p), [e[2].upper() for e in entries if len(e[2]) > 400]


@pytest.mark.parametrize("L", [64, 65, 128, 129, 160, 161, 253])
def test_fused_pass_at_the_word_count_edges_and_other_tolerances(ladder_db, L, monkeypatch):
    """k_edit_myers<W, fused> for W = ceil(L / 32) on both sides of its edges, at edit rates 0 (ED = 0: no zone between
    the thresholds), 0.04, 0.13, 0.3, 0.45 and 0.6 (2*ED > L: index.rs:406 wraps, nothing passes)"""
    ix, orc, texts = ladder_db
    ix.to_device(0)
    all_reads = helpers.ladder_reads(random.Random(3000 + L), texts, L)
    for rate in (0.0, 0.04, 0.13, 0.3, 0.45, 0.6):
        reads = few_n(all_reads, rate)
        if max(map(len, reads)) != L:  # (keeps the dispatch at this W)
            reads.append(next(r for r in all_reads if len(r) == L and n_count(r) == 0))
        assert max(map(len, reads)) == L and len(reads) > 150
        bases, off = helpers.reads_to_batch(reads)
        mp, op = both_params(edit_rate=rate)
        want, ctr = orc.bin_batch(bases, off, op, threads=8)
        assert (len(want) == 0) == (rate == 0.6)
        got, st = run_resident(ix, bases, off, mp, monkeypatch)
        check(got, st, want, ctr, rate)
        assert st["sw_diag_ms"] == 0
        if rate == 0.0:
            assert st["sw_cell_pairs"] == 0  # ED = 2*ED: the fused pass decides everything


def test_fused_pass_on_the_host_path_with_three_lanes(ladder_db, monkeypatch):
    """run_host on a batch large enough for three lanes (the oracle's answer for 3 400 distinct reads, repeated 30 times):
    every lane's slices take the fused pass, and MTSV_SW_FUSED=0 reaches the lanes too"""
    ix, orc, texts = ladder_db
    ix.to_device(0)
    rng = random.Random(35)
    unit_reads = few_n(helpers.ladder_reads(rng, texts, 150, n=1800) + helpers.ladder_reads(rng, texts, 100, n=1800))
    reps = 30
    mp, op = both_params()
    ub, uo = helpers.reads_to_batch(unit_reads)
    uwant, uctr = orc.bin_batch(ub, uo, op, threads=8)
    parts = []
    for k in range(reps):
        h = uwant.copy()
        h["read"] += k * len(unit_reads)
        parts.append(h)
    want = np.concatenate(parts)
    ctr = {k: v * reps for k, v in uctr.items()}
    bases, off = helpers.reads_to_batch(unit_reads * reps)
    assert len(off) - 1 >= 3 * 32768
    for fused in (None, "0"):
        b = make_batch(ix, len(off) - 1, len(bases), monkeypatch, fused, lanes=3)
        b.run_host(bases, off, mp)
        got, st = b.download(), b.stats()
        b.close()
        check(got, st, want, ctr, fused)
        assert st["n_lanes"] == 3
        assert (st["sw_diag_ms"] == 0) == (fused is None)
