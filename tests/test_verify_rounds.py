"""-m gpu: the verify rounds past the first.  In the reference order, for reads of up to 253 bases, a pass runs rounds of
k_edit_myers (fused) -> k_sw_pairs -> k_edit_myers (list mode); a new round starts when a list-mode lane has refused a
candidate that passed the prefilter, walked on to its TaxID's next candidate, and the two-sided bound leaves that one
undecided.  The chain databases of helpers.chain_db (shown to be what they claim by test_verify_rounds_cpu.py) hold up to
six such candidates in a row under one TaxID, so the ping-pong lists next_lists[round & 1], the count slots 11 + (round & 1),
the per-round clear mask, the tail sized from a later round's list and the "already counted" flag are all used, reused
after they were consumed, at both parities.  Every run is compared hit for hit and counter for counter with the CPU
oracle, and n_rounds with helpers.expected_rounds."""
import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import partition_ref as P
import taxa_report_ref as R
from helpers import CHAIN_CASES, assert_same_hits, chain_case, expected_rounds
from oracle import oracle as O
from test_fused_verify import both_params, check

pytestmark = pytest.mark.gpu

CASE_IDS = ["%d%s" % (L, "-N" if n else "") for L, n in CHAIN_CASES]
SWITCHES = ("MTSV_SW_FUSED", "MTSV_SW_BOUND", "MTSV_TAIL_FROM_LIST", "MTSV_FUSED_CLEAR", "MTSV_VERIFY_TURN")


class Case:
    """one chain database on the device and in the oracle, its whole batch and the oracle's answer at default parameters"""

    def __init__(self, L, with_n, tmp):
        self.db = chain_case(L, with_n)
        self.ix = M.MGIndex.build(self.db.entries, threads=4)
        p = str(tmp / ("chains_%d_%d.idx" % (L, with_n)))
        self.ix.write(p)
        self.orc = O.Index.read(p)
        self.reads = self.db.reads
        self.bases, self.off = helpers.reads_to_batch(self.reads)
        self.want, self.ctr = self.orc.bin_batch(self.bases, self.off, O.default_params(), threads=8)
        # the depth of every read the oracle showed to walk its chain as designed (None: it did not)
        self.depth = [expected_rounds(self.db.kinds_of(k)) if ok else None for k, ok in enumerate(self.db.as_predicted)]
        self.max_depth = max(d for d in self.depth if d is not None)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("chains")
    made = {}

    def get(L, with_n=False):
        if (L, with_n) not in made:
            made[(L, with_n)] = Case(L, with_n, tmp)
        made[(L, with_n)].ix.to_device(0)
        return made[(L, with_n)]

    return get


def workspace(ix, n_reads, n_bases, monkeypatch, env=None, **kw):
    """a workspace created under the given switches (they are read when it is created)"""
    for name, v in (env or {}).items():
        assert name in SWITCHES
        monkeypatch.setenv(name, v)
    try:
        return M.Batch(ix, 0, n_reads, n_bases, **kw)
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)


def run_on(b, bases, off, mp):
    b.upload(bases, off)
    b.run(mp)
    got, st = b.download(), b.stats()
    assert st["n_passes"] == 1  # n_rounds describes this pass
    return got, st


def run_resident(c, monkeypatch, mp=None, env=None, mode=None):
    b = workspace(c.ix, len(c.reads), len(c.bases), monkeypatch, env)
    if mode is not None:
        b.set_verify_mode(mode)
    got, st = run_on(b, c.bases, c.off, mp or M.default_params())
    b.close()
    return got, st


# ---- 1. the default arrangement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,with_n", CHAIN_CASES, ids=CASE_IDS)
def test_rounds_of_the_default_arrangement(cases, L, with_n, monkeypatch):
    """the whole batch of a chain database: the oracle's hits and counters, and exactly as many rounds as the deepest chain
    asks for -- six with CCCCCC + G (three in the N family, ccc): every ping-pong list and count slot is filled,
    consumed and filled again"""
    c = cases(L, with_n)
    assert c.max_depth == (3 if with_n else 6)
    assert c.ctr["n_edit"] > len(c.want) + 400 and len(c.want) > 200
    got, st = run_resident(c, monkeypatch)
    print("n_rounds", st["n_rounds"], "expected", c.max_depth)
    check(got, st, c.want, c.ctr)
    assert st["n_rounds"] == c.max_depth
    assert st["sw_diag_ms"] == 0 and st["sw_cell_pairs"] > 0  # the fused arrangement, and its sweeps ran


# ---- 2. a deep run leaves nothing behind ------------------------------------------------------------------------------
def test_sub_batches_by_depth_on_one_workspace(cases, monkeypatch):
    """the reads of the chains of depth exactly 4, 1, 3 and 2, in that order, as four batches on one workspace: the exact
    round count each time, so no list entry, count slot or cursor of a deeper run survives into a shallower one"""
    c = cases(150)
    b = workspace(c.ix, len(c.reads), len(c.bases), monkeypatch)
    mp, op = both_params()
    for d in (4, 1, 3, 2):
        reads = [r for r, k in zip(c.reads, c.depth) if k == d]
        assert len(reads) >= 6 and len(reads) % 6 == 0
        bases, off = helpers.reads_to_batch(reads)
        want, ctr = c.orc.bin_batch(bases, off, op, threads=8)
        got, st = run_on(b, bases, off, mp)
        check(got, st, want, ctr, d)
        assert st["n_rounds"] == d, d
    b.close()


# ---- 3. the other arrangements ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"MTSV_SW_FUSED": "0"}, {"MTSV_SW_BOUND": "0"}, {"MTSV_TAIL_FROM_LIST": "0"}, {"MTSV_FUSED_CLEAR": "0"},
                                 {"MTSV_TAIL_FROM_LIST": "0", "MTSV_FUSED_CLEAR": "0"}],
                         ids=["unfused", "no_bound", "tail_from_hits", "memset_clear", "tail_from_hits+memset_clear"])
def test_rounds_under_the_other_arrangements(cases, env, monkeypatch):
    """k_sw_diag in front (MTSV_SW_FUSED=0), no Myers bound (MTSV_SW_BOUND=0), every tail sized from the pass's seed hits
    (MTSV_TAIL_FROM_LIST=0) and counters cleared by memsets (MTSV_FUSED_CLEAR=0): the same hits and counters, rounds
    past the third"""
    c = cases(150)
    got, st = run_resident(c, monkeypatch, env=env)
    print("n_rounds", st["n_rounds"])
    check(got, st, c.want, c.ctr, env)
    assert st["n_rounds"] >= 4
    assert (st["sw_diag_ms"] > 0) == ("MTSV_SW_FUSED" in env or "MTSV_SW_BOUND" in env)


def test_the_edit_first_order_needs_no_rounds(cases, monkeypatch):
    c = cases(150)
    got, st = run_resident(c, monkeypatch, mode=1)
    assert_same_hits(got, c.want)
    assert st["n_rounds"] == 1


# ---- 4. cut-offs inside chains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_n", [False, True], ids=["150", "150-N"])
def test_max_candidates_inside_a_chain(cases, with_n, monkeypatch):
    """max_candidates = 1..6 ends the walk inside chains (test_verify_rounds_cpu.py): a lane, a sweep and a list lane
    must all stop at the same rank"""
    c = cases(150, with_n)
    for mc in range(1, 7):
        mp, op = both_params(max_candidates=mc)
        want, ctr = c.orc.bin_batch(c.bases, c.off, op, threads=8)
        got, st = run_resident(c, monkeypatch, mp)
        check(got, st, want, ctr, mc)


def test_max_assignments_and_other_tolerances(cases, monkeypatch):
    """max_assignments = 1 (hits only: the device verifies every chain before it cuts), and edit rates 0.12 and 0.14,
    which move the copies into other classes"""
    c = cases(150)
    mp, op = both_params(max_assignments=1)
    want, _ = c.orc.bin_batch(c.bases, c.off, op, threads=8)
    got, _ = run_resident(c, monkeypatch, mp)
    assert_same_hits(got, want)
    for rate in (0.12, 0.14):
        mp, op = both_params(edit_rate=rate)
        want, ctr = c.orc.bin_batch(c.bases, c.off, op, threads=8)
        got, st = run_resident(c, monkeypatch, mp)
        print("edit_rate", rate, "n_rounds", st["n_rounds"], "hits", len(want))
        check(got, st, want, ctr, rate)


# ---- 5. the host path, three lanes ------------------------------------------------------------------------------------
def test_rounds_on_the_host_path_with_three_lanes(cases, monkeypatch):
    """the L = 150 batch repeated until run_host has three lanes' worth of reads (the oracle's answer once, read numbers
    shifted per repetition, counters multiplied): every slice of every lane holds the deep chains, with the verify turn
    and without it"""
    c = cases(150)
    reps = -(-3 * 32768 // len(c.reads))
    parts = []
    for k in range(reps):
        h = c.want.copy()
        h["read"] += k * len(c.reads)
        parts.append(h)
    want = np.concatenate(parts)
    ctr = {k: v * reps for k, v in c.ctr.items()}
    bases, off = helpers.reads_to_batch(c.reads * reps)
    assert 3 * 32768 <= len(off) - 1 < 3 * 32768 + len(c.reads)
    for env in (None, {"MTSV_VERIFY_TURN": "0"}):
        b = workspace(c.ix, len(off) - 1, len(bases), monkeypatch, env, lanes=3)
        b.run_host(bases, off, M.default_params())
        got, st = b.download(), b.stats()
        b.close()
        print("n_rounds", st["n_rounds"], "n_passes", st["n_passes"], "verify_turns", st["verify_turns"])
        check(got, st, want, ctr, env)
        assert st["n_lanes"] == 3
        assert st["n_rounds"] >= 4
        assert (st["verify_turns"] > 0) == (env is None)


# ---- 6. match flags and the taxa report ride along --------------------------------------------------------------------
def test_match_flags_and_taxa_report_of_late_hits(cases, monkeypatch):
    """one resident run with match flags and the taxa report on: the flags and the table are those of the oracle's hits,
    so a read whose only hit arrives in round 4 or later is matched, and counted once"""
    c = cases(150)
    late = [k for k, d in enumerate(c.depth) if d is not None and d >= 4 and c.db.good_gi(k) is not None]
    assert len(late) >= 18
    b = workspace(c.ix, len(c.reads), len(c.bases), monkeypatch)
    b.set_match_flags(M.MATCH_WITH_HITS)
    b.set_taxa_report(True)
    got, st = run_on(b, c.bases, c.off, M.default_params())
    flags, n_matched = b.match_flags()
    rows, total, _ = b.taxa_report()
    b.close()
    check(got, st, c.want, c.ctr)
    assert st["n_rounds"] == c.max_depth
    want_flags = np.zeros(len(c.reads), dtype=bool)
    want_flags[c.want["read"].astype(np.int64)] = True
    assert np.array_equal(flags, want_flags) and n_matched == int(want_flags.sum())
    assert all(flags[k] for k in late)
    records = [(b"read%d" % k, b"", r, None) for k, r in enumerate(c.reads)]
    assert P.partition_by_flags(records, flags, False) == P.partition_by_flags(records, want_flags, False)
    stats, n_with_hits = R.classify_hits(c.want)
    assert R.rows_dict(rows) == stats and total == n_with_hits
    for k in late:  # its chain's TaxID is its only hit
        assert stats[c.db.chains[c.db.read_chain[k]][0]] == [6, 0, 0, 0]
