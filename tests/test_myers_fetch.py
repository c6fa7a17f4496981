"""-m gpu: the window stream of k_edit_myers.  By default the four lanes of a quad fetch one lane's 64-byte sector of the
text together, once, and hand the pieces round inside the quad; a workspace created under MTSV_MYERS_FETCH=legacy has
every lane fetch its own window, two 16-byte pieces per 16 columns.  Both must show the kernel the same columns.

Every batch runs three ways: the CPU oracle, a default workspace and a legacy one.  Hits and work counters of both
workspaces are the oracle's, and what the oracle does not count -- n_sw_passed, n_sw_bound_refuted, n_rounds,
myers_columns -- is equal between the two.  The reads' origins are placed: 72 consecutive text positions put the window's
start at every offset inside a sector (0, 1, 15, 16, 17, 47, 48, 63 among them) on both strands, origins at a sequence's
first and last bases clip the window to every length, and the N sit at chosen distances from the sector boundaries."""
import math
import os
import random

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits, revcomp
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RATE = 0.13
LENGTHS = (33, 64, 96, 150, 160, 253)       # the issue's; W = 2, 2, 3, 5, 5, 8
MORE_LENGTHS = (128, 192, 224)              # W = 4, 6, 7
VS_ORACLE = ("n_seed_hits", "n_candidates", "n_verified", "window_bytes")
VS_LEGACY = VS_ORACLE + ("n_hits", "n_sw_passed", "n_sw_bound_refuted", "n_rounds", "myers_columns")
N_AT = 8192  # text position (a multiple of 64) around which the third sequence holds its N


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


def n_sequence(rng):
    """6000 bases.  From N_AT on (a sector boundary of the text: the sequences before it hold 2 x 4000 bases): single N
    61 bases apart for 1500 bases -- a window of ~190 columns there holds three, in its first sector for some origins and
    in its last for others -- then runs of 2..12 N that straddle the sector boundaries 64 * k, a base further left each."""
    s = bytearray(helpers.rnd_seq(rng, 6000))
    at = N_AT - 8000
    for p in range(at, at + 1500, 61):
        s[p] = ord("N")
    for k, run in enumerate(range(2, 13)):
        b = at + 2048 + 320 * k
        s[b - 1 - k % run:b - 1 - k % run + run] = b"N" * run
    return bytes(s)


class Db:
    def __init__(self, entries, tmp, name):
        self.entries = entries
        self.text = helpers.geometry_text(entries)
        self.ix = M.MGIndex.build(entries, threads=4)
        self.path = str(tmp / (name + ".idx"))
        self.ix.write(self.path)
        self.orc = O.Index.read(self.path)
        self.starts = np.cumsum([0] + [len(e[2]) for e in entries]).tolist()


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """five sequences of different taxa, 22 000 symbols with the sentinel: the first starts at text position 0, the third
    holds the N, the last ends the text"""
    rng = random.Random(2828)
    seqs = [helpers.rnd_seq(rng, 4000), helpers.rnd_seq(rng, 4000), n_sequence(rng), helpers.rnd_seq(rng, 4000),
            helpers.rnd_seq(rng, 3999)]
    d = Db([(20 + k, 700 + k, s) for k, s in enumerate(seqs)], tmp_path_factory.mktemp("fetch"), "fetch")
    assert d.starts[2] == 8000 and N_AT % 64 == 0
    return d


def workspaces(ix, n_reads, n_bases, env=None, **kw):
    """(the default workspace, one created under MTSV_MYERS_FETCH=legacy), both under the switches of env"""
    assert "MTSV_MYERS_FETCH" not in os.environ
    env = dict(env or {})
    saved = {k: os.environ.get(k) for k in list(env) + ["MTSV_MYERS_FETCH"]}
    try:
        os.environ.update(env)
        new = M.Batch(ix, 0, n_reads, n_bases, **kw)
        os.environ["MTSV_MYERS_FETCH"] = "legacy"
        old = M.Batch(ix, 0, n_reads, n_bases, **kw)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return new, old


def three_ways(d, reads, env=None, passed=True, min_hits=1, rate=RATE):
    """passed: n_sw_passed is the oracle's n_edit too (the reference order, reads with at most ED N: test_fused_verify.few_n)"""
    d.ix.to_device(0)
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params(edit_rate=rate)
    want, ctr = d.orc.bin_batch(bases, off, op, threads=8)
    assert len(want) >= min_hits, len(want)
    new, old = workspaces(d.ix, len(reads), len(bases), env)
    stats = []
    try:
        for name, b in (("sectors", new), ("legacy", old)):
            b.upload(bases, off)
            b.run(mp)
            got, st = b.download(), b.stats()
            assert_same_hits(got, want)
            assert tuple(st[k] for k in VS_ORACLE) + (st["n_hits"],) == (ctr["H"], ctr["n_cand"], ctr["n_sw"], ctr["W"], len(want)), name
            if passed:
                assert st["n_sw_passed"] == ctr["n_edit"], name
            stats.append(st)
    finally:
        new.close()
        old.close()
    assert [stats[0][k] for k in VS_LEGACY] == [stats[1][k] for k in VS_LEGACY], [(k, stats[0][k], stats[1][k]) for k in VS_LEGACY]
    if "MTSV_VERIFY" not in (env or {}):  # (the edit-first order keeps no column count)
        assert stats[0]["myers_columns"] > 0
    return want, stats[0]


def cut(d, at, L, rng=None, subs=0):
    """the read of L bases whose origin is text position at, forward; with subs substitutions"""
    r = d.text[at:at + L]
    assert len(r) == L
    return helpers.substitute(rng, r, subs) if subs else r


def both_strands(reads):
    return [r if k % 2 == 0 else revcomp(r) for r in reads for k in (0, 1)]


def placed_reads(d, rng, L, lo, n=72, step=1):
    """reads of L bases at n origins from text position lo on, both strands of each: exact, with a few substitutions,
    and every third with a base left out or put in, so that the windows' ends move too"""
    ed = math.ceil(L * RATE)
    out = []
    for k in range(n):
        at = lo + k * step
        r = cut(d, at, L + 2, rng, subs=(k % 4) * ed // 5)
        if k % 3 == 1:
            r = r[:L // 2] + r[L // 2 + 1:]
        elif k % 3 == 2:
            r = r[:L // 3] + bytes([rng.choice(b"ACGT")]) + r[L // 3:]
        out.append(r[:L])
    return both_strands(out)


# ---- 1. window start offsets, read lengths ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS + MORE_LENGTHS)
def test_window_starts_at_every_offset_in_a_sector(db, L):
    """origins at 72 consecutive text positions inside the second sequence: c.x mod 64 (and c.y - 1 mod 64 of the
    reverse strand's walk) takes every value, for every W = 2..8"""
    rng = random.Random(100 + L)
    three_ways(db, placed_reads(db, rng, L, db.starts[1] + 1000 + L), min_hits=30)


# ---- 2. window lengths, text edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (64, 150))
def test_windows_clipped_at_the_first_and_last_symbol_of_the_text(db, L):
    """origins 0..79 of the first sequence (windows that start at text position 0; on the reverse strand fewer than 16 and
    fewer than 64 symbols are left above position 0 in the last blocks) and the last 80 origins of the last sequence
    (windows that end on the last symbol of the text and within its last 63): the window is clipped to a length one column
    longer from origin to origin, so lengths that are no multiple of 16 or 64, and 1..15 columns past a sector boundary"""
    rng = random.Random(200 + L)
    n = len(db.text)
    reads = placed_reads(db, rng, L, 0, n=80) + placed_reads(db, rng, L, n - L - 2 - 79, n=80)
    want, _ = three_ways(db, reads, min_hits=100)
    assert {int(g) for g in want["gi"]} >= {700, 704}


@pytest.mark.parametrize("past", (1, 15, 16, 63, 64))
def test_text_lengths_past_a_multiple_of_a_sector(tmp_path, past):
    """an index of 64 * k + past symbols (the sentinel included): reads from its last 300 and its first 100 positions"""
    rng = random.Random(300 + past)
    d = Db([(5, 50, helpers.rnd_seq(rng, 2000)), (6, 60, helpers.rnd_seq(rng, 2000)), (7, 70, helpers.rnd_seq(rng, 64 * 100 + past - 1 - 4000))],
           tmp_path, "past%d" % past)
    n = len(d.text) + 1
    assert n % 64 == past % 64
    try:
        reads = placed_reads(d, rng, 150, n - 1 - 152 - 70, n=71) + placed_reads(d, rng, 96, 0, n=40)
        three_ways(d, reads, min_hits=100)
    finally:
        d.ix.close()


# ---- 3. N ------------------------------------------------------------------------------------------------------------------
def test_windows_and_reads_with_n(db):
    """exact and substituted cuts over the single N, 61 bases apart, from 72 consecutive origins: windows with an N in
    their first and in their last sector, reads that hold N themselves facing them -- the fused lane's second pass under
    the edit distance's matches (ph = 2) -- and the same reads with their N replaced by a base, which face the window's N
    without one of their own"""
    rng = random.Random(400)
    with_n = placed_reads(db, rng, 150, N_AT + 100, n=72)
    assert all(0 < sum(c == 78 for c in r) <= 4 for r in with_n[:4])
    without = [bytes(c if c != 78 else 65 for c in r) for r in with_n]
    want, st = three_ways(db, with_n + without, min_hits=80)
    assert st["n_sw_passed"] > 0


def test_n_runs_across_sector_boundaries(db):
    """reads over the runs of 2..12 N that straddle a sector boundary, both strands, at origins 40 bases before each run
    and 8 after its start"""
    rng = random.Random(401)
    reads = []
    for k in range(11):
        b = N_AT + 2048 + 320 * k
        for at in (b - 110, b - 70, b - 40, b - 6):
            reads += both_strands([cut(db, at, 150, rng, subs=k % 3)])
    three_ways(db, reads, min_hits=20)


# ---- 4. the other modes of the kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("env,passed", [({"MTSV_SW_FUSED": "0"}, True), ({"MTSV_VERIFY": "edit_first"}, False)], ids=["bound+list", "chain"])
def test_bound_list_and_chain_mode(db, env, passed):
    """MTSV_SW_FUSED=0: k_sw_diag, then k_edit_myers as the bound, the sweep, k_edit_myers in list mode.
    MTSV_VERIFY=edit_first: k_edit_myers alone, walking the chains of a TaxID itself"""
    rng = random.Random(500)
    reads = placed_reads(db, rng, 150, db.starts[3] + 700, n=72) + placed_reads(db, rng, 150, N_AT + 100, n=24, step=3)
    three_ways(db, reads, env=env, passed=passed, min_hits=80)


# ---- 5. partial waves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 2, 3, 5, 61))
def test_fewer_work_items_than_a_wavefront(db, count):
    """1, 2, 3, 5 and 61 reads, a candidate each at most: quads in which one, two or three lanes have a window and the others
    fetch for them, and wavefronts with whole quads idle"""
    rng = random.Random(600 + count)
    reads = placed_reads(db, rng, 150, db.starts[1] + 333, n=64, step=7)[:count]
    want, st = three_ways(db, reads, min_hits=1)
    assert 1 <= st["n_candidates"] < 64  # (a read whose substitutions left it no seed has no candidate)


# ---- 6. chains ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_n", (False, True), ids=["ACGT", "N"])
def test_lanes_that_walk_on_to_new_windows(tmp_path, with_n):
    """helpers.chain_case(150): up to six candidates in a row under one TaxID; a lane that refutes one walks on to the next,
    a new window at another place of the text, while its quad neighbours are in the middle of theirs"""
    c = helpers.chain_case(150, with_n)
    d = Db(c.entries, tmp_path, "chains")
    try:
        want, st = three_ways(d, c.reads, min_hits=200)
        assert st["n_rounds"] == max(helpers.expected_rounds(c.kinds_of(k)) for k, ok in enumerate(c.as_predicted) if ok)
        three_ways(d, c.reads, env={"MTSV_VERIFY": "edit_first"}, passed=False, min_hits=200)
    finally:
        d.ix.close()


# ---- 7. the text on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past", (1, 16, 63, 64))
def test_both_uploads_pad_the_text_to_whole_sectors(tmp_path, past):
    """the host pack and the device pack leave the same bytes: the codes, then 7 up to the end of the sector and one
    sector more; MTSV_DEVPART_TEXT is its first (n + 15) / 16 * 16 + 32 bytes as before"""
    rng = random.Random(700 + past)
    d = Db([(5, 50, helpers.rnd_seq(rng, 3000, b"ACGTN")), (6, 60, helpers.rnd_seq(rng, 64 * 80 + past - 1 - 3000))], tmp_path, "pad%d" % past)
    n = len(d.text) + 1
    assert n % 64 == past % 64
    host, dev = M.MGIndex.load(d.path), M.MGIndex.load(d.path)
    try:
        host.to_device(0, M.DEV_DEFAULT)
        dev.to_device(0, M.DEV_PACK_ON_DEVICE)
        a, b = host.download_device(0, M.DEVPART_TEXT_SECTORS), dev.download_device(0, M.DEVPART_TEXT_SECTORS)
        assert len(a) == (n + 63) // 64 * 64 + 64 and a == b
        assert set(a[n:]) == {7} and 7 not in set(a[:n])
        short = host.download_device(0, M.DEVPART_TEXT)
        assert short == dev.download_device(0, M.DEVPART_TEXT) == a[:(n + 15) // 16 * 16 + 32]
        assert host.info() == dev.info()
    finally:
        host.close()
        dev.close()
        d.ix.close()
