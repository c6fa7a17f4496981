"""-m gpu: the lane policies of a workspace of several lanes ("Lanes").  k_edit_myers takes a grid of
256 x R workgroups (MTSV_MYERS_WGS_PER_CU), one lane at a time has the verify kernels of a pass in flight (the verify turn,
MTSV_VERIFY_TURN), and the tail of a verify round is sized from its own list.  None of this may change a hit or a counter:
every batch here is large enough for three lanes (98 304 reads or more), runs on the resident path and on the host path, and
is compared field for field with the CPU oracle.  The turn must come back from a lane that throws, and a lane without work
must never wait for it."""
import random
import threading

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("n_candidates", "n_verified", "window_bytes", "n_sw_passed", "n_hits")
SWITCHES = ("MTSV_MYERS_WGS_PER_CU", "MTSV_VERIFY_TURN")
MIN_READS = 3 * 32768
DEADLINE_S = 120  # a run of 100 000 short reads takes well under a second: beyond this a lane is waiting for a turn that never comes


def few_n(reads, edit_rate=0.13):
    """(as in test_fused_verify.py: a read with more N than edits allowed never reaches the verify kernels)"""
    import math
    return [r for r in reads if sum(c not in b"ACGTacgt" for c in r) <= math.ceil(len(r) * edit_rate)]


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    entries, _, _ = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "lane_overlap.idx")
    ix.write(p)
    return ix, O.Index.read(p), entries


def repeated(orc, op, blocks):
    """blocks: [(reads, repetitions)].  The batch of every block's reads repeated in turn, and the oracle's answer for it,
    computed once per block"""
    reads, parts, ctr, base = [], [], {}, 0
    for unit, reps in blocks:
        ub, uo = helpers.reads_to_batch(unit)
        uwant, uctr = orc.bin_batch(ub, uo, op, threads=8)
        for _ in range(reps):
            h = uwant.copy()
            h["read"] += base
            parts.append(h)
            base += len(unit)
        reads += unit * reps
        for k, v in uctr.items():
            ctr[k] = ctr.get(k, 0) + v * reps
    bases, off = helpers.reads_to_batch(reads)
    return bases, off, np.concatenate(parts), ctr


def make_batch(ix, n_reads, n_bases, monkeypatch, wgs=None, turn=None):
    """a three-lane workspace; the switches are read when it is created"""
    for name, v in zip(SWITCHES, (wgs, turn)):
        if v is not None:
            monkeypatch.setenv(name, str(v))
    try:
        return M.Batch(ix, 0, n_reads, n_bases, lanes=3)
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)


HUNG = []  # a call that did not come back: its thread is still inside the library, its workspace must not be touched again


def close(b):
    """closes the workspace, unless a call is still running somewhere in this process (which ends with the failure instead)"""
    if not HUNG:
        b.close()


def within_deadline(fn):
    """fn() on a thread of its own (the library calls release the interpreter): its result, its exception, or a failure when
    it has not come back in time"""
    assert not HUNG, "an earlier call never came back"
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001 (handed to the caller)
            box["error"] = e

    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(DEADLINE_S)
    if t.is_alive():
        HUNG.append(t)
    assert not t.is_alive(), f"no answer within {DEADLINE_S} s: a lane is waiting"
    if "error" in box:
        raise box["error"]
    return box["value"]


def check(b, want, ctr, what, wgs=None, turn=None):
    """the oracle's hits and counters; and, where the switches are known, that they reached the launches: no k_edit_myers
    grid beyond 256 x wgs workgroups, every pass with seed hits took the turn and no two lanes were in their verify
    sections at once (turn on), nobody took it (turn off)"""
    got, st = b.download(), b.stats()
    assert_same_hits(got, want)
    assert tuple(st[k] for k in COUNTERS) == (ctr["n_cand"], ctr["n_sw"], ctr["W"], ctr["n_edit"], len(want)), what
    assert st["n_lanes"] == 3, what
    if wgs is not None:
        assert 16 <= st["myers_grid_max"] <= 256 * wgs, (what, st["myers_grid_max"])
    if turn == 1:
        assert 1 <= st["verify_turns"] <= st["n_passes"] and st["verify_lanes_max"] == 1, (what, st["verify_turns"], st["verify_lanes_max"])
    elif turn == 0:
        assert st["verify_turns"] == 0 and st["verify_lanes_max"] >= 1, (what, st["verify_turns"], st["verify_lanes_max"])


@pytest.fixture(scope="module")
def mixed_batch(db):
    ix, orc, entries = db
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    rng = random.Random(41)
    unit = few_n(helpers.ladder_reads(rng, texts, 150, n=1800) + helpers.ladder_reads(rng, texts, 100, n=1800))
    reps = -(-MIN_READS // len(unit))
    op = O.default_params()
    bases, off, want, ctr = repeated(orc, op, [(unit, reps)])
    assert len(off) - 1 >= MIN_READS and len(want) > 1000
    return bases, off, want, ctr


@pytest.mark.parametrize("turn", [0, 1])
@pytest.mark.parametrize("wgs", [2, 3, 5])
def test_grid_cap_and_turn_change_no_hit_and_no_counter(db, mixed_batch, wgs, turn, monkeypatch):
    """MTSV_MYERS_WGS_PER_CU in {2, 3, 5} x MTSV_VERIFY_TURN in {0, 1}: the resident path and the host path return the
    oracle's hits and counters"""
    ix, _, _ = db
    ix.to_device(0)
    bases, off, want, ctr = mixed_batch
    mp = M.default_params()
    b = make_batch(ix, len(off) - 1, len(bases), monkeypatch, wgs, turn)
    try:
        b.upload(bases, off)
        within_deadline(lambda: b.run(mp))
        check(b, want, ctr, ("resident", wgs, turn), wgs, turn)
        within_deadline(lambda: b.run_host(bases, off, mp))
        check(b, want, ctr, ("host", wgs, turn), wgs, turn)
    finally:
        close(b)


def test_defaults_on_both_paths(db, mixed_batch, monkeypatch):
    """the same with no switch set: what a caller gets"""
    ix, _, _ = db
    ix.to_device(0)
    bases, off, want, ctr = mixed_batch
    mp = M.default_params()
    b = make_batch(ix, len(off) - 1, len(bases), monkeypatch)
    try:
        b.upload(bases, off)
        within_deadline(lambda: b.run(mp))
        check(b, want, ctr, "resident", 3, 1)  # (the defaults of a workspace of several lanes)
        within_deadline(lambda: b.run_host(bases, off, mp))
        check(b, want, ctr, "host", 3, 1)
    finally:
        close(b)


def test_a_lane_that_throws_gives_the_turn_back(db, mixed_batch, monkeypatch):
    """a host batch with one read beyond 32 767 bases: the lane that meets it raises the `limit:` error while the others are
    in their passes (holding or waiting for the turn); the call raises, and the next calls on the same workspace complete
    with the right hits.  The error is raised before the lane's pass takes the turn, so what this shows is that a run that
    ends in an error leaves no turn held and no lane waiting; the guard's release inside a pass is by scope (batch.hip)"""
    ix, _, _ = db
    ix.to_device(0)
    bases, off, want, ctr = mixed_batch
    mp = M.default_params()
    n = len(off) - 1
    at = 2 * n // 3  # the long read: inside the batch, where another lane has passes before and after it
    long_read = np.frombuffer(helpers.rnd_seq(random.Random(42), 40000), dtype=np.uint8)
    cut = int(off[at])
    bad_bases = np.concatenate([bases[:cut], long_read, bases[cut:]])
    bad_off = np.concatenate([off[:at + 1], off[at:] + np.uint64(len(long_read))]).astype(np.uint64)
    assert len(bad_off) == n + 2 and int(bad_off[at + 1] - bad_off[at]) == 40000
    b = make_batch(ix, n + 1, len(bad_bases), monkeypatch, turn=1)
    try:
        with pytest.raises(M.MtsvError, match="limit:"):
            within_deadline(lambda: b.run_host(bad_bases, bad_off, mp))
        within_deadline(lambda: b.run_host(bases, off, mp))
        check(b, want, ctr, "host, after the error", turn=1)
        b.upload(bases, off)
        within_deadline(lambda: b.run(mp))
        check(b, want, ctr, "resident, after the error", turn=1)
    finally:
        close(b)


def test_lanes_without_work_do_not_wait_for_the_turn(db, monkeypatch):
    """reads of one taxon, then twice as many reads that hit nothing: every work item sits in the first lane's range, the
    other lanes' passes have no seed hit, and the batch completes on both paths"""
    ix, orc, entries = db
    ix.to_device(0)
    rng = random.Random(43)
    text = max((e[2].upper() for e in entries if e[0] == 77), key=len)
    hitting = []
    for _ in range(2048):
        st = rng.randrange(0, len(text) - 150)
        r = helpers.substitute(rng, text[st:st + 150], rng.randrange(0, 6))
        hitting.append(r if rng.random() < 0.5 else helpers.revcomp(r))
    hitting = few_n(hitting)
    junk = [helpers.rnd_seq(rng, 150) for _ in range(2048)]
    op = O.default_params()
    bases, off, want, ctr = repeated(orc, op, [(hitting, -(-32768 // len(hitting))), (junk, 32)])
    n = len(off) - 1
    assert n >= MIN_READS
    assert len(want) > 8192
    mp = M.default_params()
    b = make_batch(ix, n, len(bases), monkeypatch, turn=1)
    try:
        b.upload(bases, off)
        within_deadline(lambda: b.run(mp))
        check(b, want, ctr, "resident")
        within_deadline(lambda: b.run_host(bases, off, mp))
        check(b, want, ctr, "host")
    finally:
        close(b)
