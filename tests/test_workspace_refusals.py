"""-m gpu: a device allocation that is refused while a workspace grows leaves the workspace usable.

MTSV_ALLOC_REFUSE names an array of the workspace (csrc/dev_mem.hpp: the allocation throws what a refused hipMalloc throws,
without a call to the runtime; no test may exhaust the memory of a shared card).  Every case runs four steps on one handle:
inputs A; inputs B, which need the named array to grow, with the knob set -- the call fails with "device: no memory for";
B again with the knob cleared; A again.  What the handle returns in steps 1, 3 and 4 is compared with what a fresh workspace
returns for the same inputs, never with anything the handle itself returned.  A growth that left a capacity above zero over
released arrays would put a null array under a kernel of step 3 or 4.

The arrays that keep their contents when they grow (the result array, the assignments) leave the handle as it was when the
allocation is refused; a run that fails has already dropped the results of the run before it (begin_run), so that the old
array was not lost shows in steps 3 and 4 only."""
import random

import pytest

import helpers
import mtsv_tools_amd as M

pytestmark = pytest.mark.gpu

KNOB = "MTSV_ALLOC_REFUSE"
LANES = [1, 2]
# (a workspace of fewer than 32768 reads per lane is created with one lane)
SIZE = {1: (4400, 4400 * 330), 2: (65536, 65536 * 16)}


@pytest.fixture(scope="module")
def db():
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    rng = random.Random(411)
    plain = [e[2] for e in entries if len(e[2]) > 1500 and set(e[2]) <= set(b"ACGT")]

    def cuts(n, length):
        out = []
        for k in range(n):
            t = plain[k % len(plain)]
            st = rng.randrange(0, len(t) - length)
            r = helpers.mutate(rng, t[st:st + length], k % 4, b"ACGT")
            out.append(r if k % 2 else helpers.revcomp(r))
        return out

    gene_reads = [helpers.mutate(rng, gene[st:st + 150], k % 5, b"ACGT") for k, st in enumerate(range(0, 540, 3))]  # (8 hits each)
    yield {"ix": ix, "short": cuts(40, 50), "long": cuts(40, 150), "many": cuts(130, 50), "gene": gene_reads,
           "repeat": cuts(9, 100) + [(unit * 5)[20:170]]}
    ix.close()


class Setup:
    """how the workspaces of a case are made and switched, the handle under test and the fresh ones alike"""

    def __init__(self, lanes, hit_ws=0, env=None, flags=False, host=False, size=None):
        self.lanes, self.hit_ws, self.env, self.flags, self.host = lanes, hit_ws, env or {}, flags, host
        self.size = size or SIZE[lanes]

    def make(self, ix, monkeypatch):
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        b = M.Batch(ix, 0, *self.size, self.hit_ws, lanes=self.lanes)
        if self.flags:
            b.set_match_flags(M.MATCH_WITH_HITS)
        return b

    def run(self, b, reads, assign=False):
        b.set_assignments(M.ASSIGN_WITH_HITS if assign else M.ASSIGN_OFF)
        if self.host:
            b.run_host(*helpers.reads_to_batch(reads))
        else:
            b.upload(*helpers.reads_to_batch(reads))
            b.run()
        return observe(b, assign, self.flags)


def observe(b, assign, flags):
    out = {"hits": b.download()}
    if assign:
        out["assign"] = b.download_assignments()[0].tobytes()
    if flags:
        f, matched = b.match_flags()
        out["flags"] = (f.tolist(), matched)
    return out


def same(got, want, what):
    helpers.assert_same_hits(got["hits"], want["hits"])
    for k in ("assign", "flags"):
        assert (k in got) == (k in want) and got.get(k) == want.get(k), (what, k)


def refused(call, what):
    with pytest.raises(M.MtsvError) as e:
        call()
    assert str(e.value).split(": ", 1)[1].startswith("device: no memory for"), str(e.value)
    assert what in str(e.value), str(e.value)


def four_steps(db, monkeypatch, setup, what, a, b, assign_b=False):
    ix = db["ix"]
    fresh = {}
    for name, reads, assign in (("a", a, False), ("b", b, assign_b), ("a_again", a, assign_b)):
        w = setup.make(ix, monkeypatch)
        fresh[name] = setup.run(w, reads, assign)
        w.close()
    assert len(fresh["a"]["hits"]) and len(fresh["b"]["hits"])
    ws = setup.make(ix, monkeypatch)
    try:
        same(setup.run(ws, a), fresh["a"], "step 1")
        monkeypatch.setenv(KNOB, what)
        refused(lambda: setup.run(ws, b, assign_b), what)
        monkeypatch.delenv(KNOB)
        same(setup.run(ws, b, assign_b), fresh["b"], "step 3")
        same(setup.run(ws, a, assign_b), fresh["a_again"], "step 4")
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        ws.close()


@pytest.mark.parametrize("what", ["seed slots: ranges", "seed slots: prefix sums", "the reads' bit planes"])
def test_seed_slots_and_planes(db, monkeypatch, what):
    """50-base reads, then 150-base reads: more seed slots per read and wider bit planes.  Both arrays are sized for a full
    workspace of reads like the first pass's, so they grow again only where 40 reads of 150 bases need more than a workspace
    of 50-base reads: a workspace of 48 reads, which has one lane (a lane holds 32768 reads or more, and with them room
    that tens of reads never exceed)"""
    four_steps(db, monkeypatch, Setup(1, size=(48, 48 * 330)), what, db["short"], db["long"])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("what", ["hit workspace: rows", "hit workspace: work list"])
def test_hit_workspace(db, monkeypatch, lanes, what):
    """a workspace of 64 seed hits and a read of a tandem repeat, which alone has more: the first and the last of the ten
    arrays refused (the last: nine of them exist at the new size when the growth fails)"""
    four_steps(db, monkeypatch, Setup(lanes, hit_ws=64), what, db["short"][:10], db["repeat"])


@pytest.mark.parametrize("lanes", LANES)
def test_result_array(db, monkeypatch, lanes):
    """a result array of 1024 hits and a workspace of 2048 seed hits: the 180 reads of the conserved gene (1440 hits) run in several
    passes, and the array grows behind the hits of the first ones, which it keeps"""
    four_steps(db, monkeypatch, Setup(lanes, hit_ws=2048, env={"MTSV_HITS_CAP": "1024"}), "the result array", db["short"], db["gene"])
    # (what the case relies on)
    setup = Setup(lanes, hit_ws=2048, env={"MTSV_HITS_CAP": "1024"})
    w = setup.make(db["ix"], monkeypatch)
    got = setup.run(w, db["gene"])
    assert len(got["hits"]) > 1024 and w.stats()["n_passes"] > 1
    w.close()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("what", ["collapse scratch: keys", "collapse scratch: tile sums", "collapse scratch: read list", "the assignments"])
def test_collapse_and_assignments(db, monkeypatch, lanes, what):
    """A runs with the assignments off, B is the workspace's first run with them on: the collapse scratch and the assignment
    array are created (at their floors, which tens of reads never exceed); hits and assignments are compared"""
    four_steps(db, monkeypatch, Setup(lanes), what, db["short"], db["gene"][:40], assign_b=True)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("what", ["arena 0: bases", "arena 0: packed bases", "arena 0: offsets"])
def test_arena(db, monkeypatch, lanes, what):
    """host batches with the input segments at their floor: 2000 bases, then 6000"""
    four_steps(db, monkeypatch, Setup(lanes, env={"MTSV_ARENA_BASES": "65536"}, host=True), what, db["short"], db["long"])


@pytest.mark.parametrize("lanes", LANES)
def test_match_flags(db, monkeypatch, lanes):
    """40 reads need one word of flags, 130 need three"""
    four_steps(db, monkeypatch, Setup(lanes, flags=True), "the match flags", db["short"], db["many"])


@pytest.mark.parametrize("lanes", LANES)
def test_compaction(db, monkeypatch, lanes):
    """take_reads creates the compaction's tile sums; the destination is the handle under test"""
    ix = db["ix"]
    setup = Setup(lanes)
    a, b = db["short"], db["long"][:20] + [helpers.rnd_seq(random.Random(5), 150) for _ in range(20)]
    src = Setup(lanes, flags=True).make(ix, monkeypatch)
    src.upload(*helpers.reads_to_batch(b))
    src.run()

    def taken(w):
        n, nb, _ = w.take_reads(src, M.KEEP_MATCHED)
        w.run()
        return n, nb, w.read_map().tolist(), observe(w, False, False)

    w = setup.make(ix, monkeypatch)
    want_a = setup.run(w, a)
    w.close()
    w = setup.make(ix, monkeypatch)
    want_b = taken(w)
    w.close()
    assert 0 < want_b[0] < len(b) and len(want_b[3]["hits"])
    ws = setup.make(ix, monkeypatch)
    try:
        same(setup.run(ws, a), want_a, "step 1")
        monkeypatch.setenv(KNOB, "the compaction's tile sums")
        refused(lambda: ws.take_reads(src, M.KEEP_MATCHED), "the compaction's tile sums")
        monkeypatch.delenv(KNOB)
        got = taken(ws)
        assert got[:3] == want_b[:3]
        same(got[3], want_b[3], "step 3")
        same(setup.run(ws, a), want_a, "step 4")
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        ws.close()
        src.close()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("what", ["the result array", "hit workspace: status"])
def test_constructor(db, monkeypatch, lanes, what):
    """an array allocated late in the constructor is refused: mtsv_batch_create returns the error (every member created
    before it frees itself), and the next workspace runs A"""
    setup = Setup(lanes)
    w = setup.make(db["ix"], monkeypatch)
    want = setup.run(w, db["short"])
    w.close()
    monkeypatch.setenv(KNOB, what)
    refused(lambda: setup.make(db["ix"], monkeypatch), what)
    monkeypatch.delenv(KNOB)
    ws = setup.make(db["ix"], monkeypatch)
    try:
        same(setup.run(ws, db["short"]), want, "after the refused constructor")
    finally:
        ws.close()
