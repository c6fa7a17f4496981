"""-m gpu: the reads' bit planes.  k_thin writes three planes per read with a seed hit (bit 0 and bit 1 of the base code,
"is N"), Wp = the pass's word count per plane, read-relative; k_edit_myers (fused, bound, list and chain mode) sets up its
match masks from them with a funnel shift by 32*W - L and takes the read's N count from the N plane's population count.
The cases sit where that can go wrong: read lengths on both sides of every 32-row word edge in mixed-length batches (reads
start at every byte offset modulo 16, Wp exceeds a read's own word count), N at a read's ends and beside its word edges, N
counts at the tolerance's edge, reads without an image between reads with one, lanes and ranges of a host batch.  Every
batch is compared hit for hit with the CPU oracle and its work counters with the oracle's, through the C ABI, in the
reference order, the edit-first order and with MTSV_SW_FUSED=0."""
import math
import random

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EDGES = [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 253]
RATE = 0.13


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    entries, _, _ = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "planes.idx")
    ix.write(p)
    ix.to_device(0)
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    texts = [bytes(c if c in b"ACGT" else 65 for c in t) for t in texts]  # the reads' only N are the planted ones
    return ix, O.Index.read(p), texts


def ed_of(L, rate=RATE):
    return math.ceil(L * rate)


def n_count(r):
    return sum(c not in b"ACGT" for c in r)


def with_n(r, positions):
    r = bytearray(r)
    for q in positions:
        r[q] = ord("N")
    return bytes(r)


def origin(rng, texts, L):
    t = rng.choice([t for t in texts if len(t) >= L + 60])
    st = rng.randrange(0, len(t) - L - 20)
    return t[st:st + L + 20]


def edge_reads(rng, texts, L, n):
    """n reads of exactly L bases from the database, both strands: exact, substituted, with indels, N at the first and the
    last base, N on both sides of the plane words' edges (read positions 32j - 1, 32j) and of the row words' edges of a
    kernel of any W (positions L - 32j - 1, L - 32j: the read sits at the top of the rows)"""
    ed = ed_of(L)
    reads = []
    for i in range(n):
        seg = origin(rng, texts, L)
        kind = i % 6
        if kind == 0:
            r = seg[:L]
        elif kind == 1:
            r = helpers.substitute(rng, seg[:L], rng.randrange(0, ed + 2))
        elif kind == 2:
            r = helpers.mutate(rng, seg, rng.randrange(1, ed + 1), b"ACGT")[:L]
            r = r + seg[len(r):L]
        elif kind == 3:
            r = with_n(seg[:L], [0, L - 1][:ed])
        elif kind == 4:
            at = [q for j in range(1, 8) for q in (32 * j - 1, 32 * j) if q < L]
            r = with_n(seg[:L], rng.sample(at, min(len(at), ed, 4)) if at else [0])
        else:
            at = [q for j in range(1, 8) for q in (L - 32 * j - 1, L - 32 * j) if q >= 0]
            r = with_n(helpers.substitute(rng, seg[:L], 1), rng.sample(at, min(len(at), ed - 1, 4)) if at else [L - 1])
        assert len(r) == L
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    return reads


def arrangements(ix, n_reads, n_bases, monkeypatch, **kw):
    """(name, workspace, verify mode): the reference order (round 0 fused), edit-first, the reference order unfused"""
    b = M.Batch(ix, 0, n_reads, n_bases, **kw)
    monkeypatch.setenv("MTSV_SW_FUSED", "0")
    try:
        bu = M.Batch(ix, 0, n_reads, n_bases, **kw)
    finally:
        monkeypatch.delenv("MTSV_SW_FUSED", raising=False)
    return (("reference", b, 0), ("edit_first", b, 1), ("unfused", bu, 0))


def check(got, st, want, ctr, what, passed=True):
    """all six hit fields and the work counters.  passed: n_sw_passed too -- the reference order on reads with at most ED
    N (the strands of a read with more never reach the verify kernels, which therefore do not count what the prefilter
    would have passed for them: tests/test_fused_verify.py, few_n)"""
    assert_same_hits(got, want)
    assert (st["n_seed_hits"], st["n_candidates"]) == (ctr["H"], ctr["n_cand"]), what
    assert (st["n_verified"], st["window_bytes"], st["n_hits"]) == (ctr["n_sw"], ctr["W"], len(want)), what
    if passed:
        assert st["n_sw_passed"] == ctr["n_edit"], what


def run_all(db, reads, monkeypatch, few_n=True, rate=RATE, min_hits=1):
    ix, orc, _ = db
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params(edit_rate=rate)
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    assert len(want) >= min_hits, len(want)
    for name, b, mode in arrangements(ix, len(reads), len(bases), monkeypatch):
        b.set_verify_mode(mode)
        b.upload(bases, off)
        b.run(mp)
        check(b.download(), b.stats(), want, ctr, name, passed=few_n and mode == 0)
        if name != "reference":  # (edit-first runs on the reference order's workspace)
            b.close()
    return want


# ---- 1. word edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lmax", EDGES)
def test_lengths_at_every_word_edge_in_mixed_batches(db, Lmax, monkeypatch):
    """a pass whose longest read has Lmax bases (that picks W and Wp) and holds every shorter length of the list next to
    it, shuffled: the reads start at every byte offset modulo 16, and the short ones own fewer words than Wp"""
    _, _, texts = db
    rng = random.Random(4000 + Lmax)
    reads = edge_reads(rng, texts, Lmax, 24)
    for L in EDGES:
        if L < Lmax:
            reads += edge_reads(rng, texts, L, 6)
    rng.shuffle(reads)
    assert max(map(len, reads)) == Lmax
    if Lmax == 253:
        assert {off % 16 for off in np.cumsum([0] + [len(r) for r in reads])} == set(range(16))
    want = run_all(db, reads, monkeypatch, min_hits=len(reads) // 3)
    assert {0, 1} <= set(want["strand"].tolist())


# ---- 2. N at the ends and at the tolerance's edge ----------------------------------------------------------------------
@pytest.mark.parametrize("L", [33, 64, 97, 150, 160, 225, 253])
def test_n_counts_at_the_tolerance_edge(db, L, monkeypatch):
    """exactly ED and ED + 1 N in an otherwise exact read, scattered, packed at the read's start, at its end and around a
    word edge: the first kind is accepted with edit = ED, the second is hopeless -- a population count decides.  And a
    read made only of N."""
    _, _, texts = db
    rng = random.Random(5000 + L)
    ed = ed_of(L)
    reads, accept = [], 0
    for i in range(48):
        seg = origin(rng, texts, L)[:L]
        k = ed + (i & 1)
        how = (i >> 1) % 4
        if how == 0:
            at = rng.sample(range(L), k)
        elif how == 1:
            at = range(k)
        elif how == 2:
            at = range(L - k, L)
        else:
            lo = max(0, min(L - k, 32 * rng.randrange(1, (L + 31) // 32) - k // 2))
            at = range(lo, lo + k)
        r = with_n(seg, at)
        assert n_count(r) == k
        reads.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    reads += [b"N" * L, b"N" * 31, origin(rng, texts, L)[:L]]
    rng.shuffle(reads)
    assert max(map(len, reads)) == L
    want = run_all(db, reads, monkeypatch, few_n=False, min_hits=8)
    by_read = {}
    for h in want:
        by_read.setdefault(int(h["read"]), []).append(int(h["edit"]))
    for i, r in enumerate(reads):
        if n_count(r) > ed_of(len(r)):
            assert i not in by_read
        elif i in by_read and n_count(r):
            assert min(by_read[i]) == n_count(r) == ed
    # without the hopeless reads: n_sw_passed as well
    run_all(db, [r for r in reads if n_count(r) <= ed_of(len(r))], monkeypatch, min_hits=8)


# ---- 3. reads without an image between reads with one -------------------------------------------------------------------
def test_most_reads_have_no_seed_hit(db, monkeypatch):
    """nine reads in ten are random sequence without a seed hit: k_thin writes them no image, and the images of the
    others sit at their reads' own places"""
    _, _, texts = db
    rng = random.Random(6000)
    reads = []
    for i in range(1500):
        L = rng.choice(EDGES[3:])
        if i % 10 == 3:
            reads += edge_reads(rng, texts, L, 1)
        else:
            reads.append(helpers.rnd_seq(rng, L))
    want = run_all(db, reads, monkeypatch, min_hits=100)
    assert len(set(want["read"].tolist())) < 200


# ---- 4. lanes and ranges -------------------------------------------------------------------------------------------------
def test_three_lanes_and_several_ranges_keep_their_images_apart(db, monkeypatch):
    """run_host on 200 000 reads through a workspace of 98 304: three lanes, several ranges.  The batch is 1 699 distinct
    reads of mixed lengths (one in four without a seed hit), repeated: a lane that read another lane's or an earlier
    pass's image would set up another read's masks, since no lane or range boundary is a multiple of 1 699"""
    ix, orc, texts = db
    rng = random.Random(7000)
    unit = []
    while len(unit) < 1699:
        L = rng.choice(EDGES[3:] + [150] * 8)
        unit += [helpers.rnd_seq(rng, L)] if len(unit) % 4 == 1 else edge_reads(rng, texts, L, 1)
    reps = 120
    mp, op = both_params(edit_rate=RATE)
    ub, uo = helpers.reads_to_batch(unit)
    uwant, uctr = orc.bin_batch(ub, uo, op, threads=8)
    assert len(uwant) > 1000
    parts = []
    for k in range(reps):
        h = uwant.copy()
        h["read"] += k * len(unit)
        parts.append(h)
    want = np.concatenate(parts)
    ctr = {k: v * reps for k, v in uctr.items()}
    bases, off = helpers.reads_to_batch(unit * reps)
    n = len(off) - 1
    assert n > 2 * 98304
    for name, b, mode in arrangements(ix, 98304, 98304 * 160, monkeypatch, lanes=3):
        b.set_verify_mode(mode)
        b.run_host(bases, off, mp)
        got, st = b.download(), b.stats()
        check(got, st, want, ctr, name, passed=mode == 0)
        assert st["n_lanes"] == 3 and st["n_passes"] >= 6, (name, st["n_lanes"], st["n_passes"])
        if name != "reference":
            b.close()
