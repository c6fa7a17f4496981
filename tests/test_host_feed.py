"""-m gpu test of a host run whose input lies in parts AND in several input segments while both pinned stages fill
(Batch::HostRun in batch_host.hip, the cursor of host_feed.hpp, PinnedStage): one run_host_parts call on the adversarial
reads, cut into four parts -- one empty, one page-locked --, with input segments so small that segment boundaries fall inside
parts and part boundaries inside segments; packed and plain transfer; hits alone, hits and assignments at the TaxID grain and
at the (TaxID, GI) grain, every run twice on its workspace so that the second begins from the stages' last totals.

One lane: the 575 reads on a workspace of 97 reads.  Two lanes: a workspace runs a host batch on a second lane only from
2 x 32,768 reads on (kLaneMinReads), so that case puts 2 x 32,768 - 575 reads of random bases, which hit nothing and cost
little, between two copies of the 575 reads -- 66,111 reads in well over a hundred segments on a workspace that holds them
all -- and asserts that two lanes worked: a second lane's thread, and ranges that finish out of order, since a segment of
the adversarial reads takes many times as long as one of the random ones.

Only the CPU oracle decides what is expected, run on each case's own input."""
import numpy as np
import pytest

import assign_ref as A
import grain_ref as GR
import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ARENA_BASES = 65536
LANE_MIN_READS = 32768              # kLaneMinReads of pass_plan.hpp
CUTS = {1: (0, 200, 200, 400), 2: (0, 20_000, 20_000, 45_000)}     # reads: part 1 is empty, part 2 page-locked


def in_parts(bases, off, cuts):
    """(parts, the page-locked buffer); asserts the geometry the test is about: where the feeder closes its segments (the
    next read does not fit) against the cuts"""
    n = len(off) - 1
    cuts = list(cuts) + [n]
    segs = [0]
    for r in range(n):
        if int(off[r + 1] - off[segs[-1]]) > ARENA_BASES:
            segs.append(r)
    assert len(segs) >= 2
    assert any(a < s < c for s in segs[1:] for a, c in zip(cuts, cuts[1:])), "no segment boundary inside a part"
    assert any(a < c < e for c in cuts[1:-1] for a, e in zip(segs, segs[1:] + [n])), "no part boundary inside a segment"
    hb = M.HostBuffer(int(off[cuts[3]] - off[cuts[2]]))
    hb.array[:] = bases[int(off[cuts[2]]):int(off[cuts[3]])]
    parts = [(hb.array if k == 2 else bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a]) for k, (a, c) in enumerate(zip(cuts, cuts[1:]))]
    assert len(parts) == 4 and len(parts[1][1]) == 1
    return parts, hb


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.to_device(0)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=50, lengths=(100, 150, 64, 253))
    bases, off = helpers.reads_to_batch(reads)
    n = len(reads)
    want, _ = O.Index.read(p).bin_batch(bases, off, O.default_params(), threads=8)
    assert len(want) > 100
    rng = np.random.default_rng(5)
    lens = rng.integers(100, 151, size=2 * LANE_MIN_READS - n)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lens.sum()))].tobytes()
    ends = np.cumsum(lens).tolist()
    filler = [letters[e - l:e] for e, l in zip(ends, lens.tolist())]
    big_bases, big_off = helpers.reads_to_batch(reads + filler + reads)
    big_want, _ = O.Index.read(p).bin_batch(big_bases, big_off, O.default_params(), threads=8)
    assert len(big_want) == 2 * len(want)               # (the random reads hit nothing)
    by_lanes, buffers = {}, []
    for lanes, (b, o, w) in {1: (bases, off, want), 2: (big_bases, big_off, big_want)}.items():
        parts, hb = in_parts(b, o, CUTS[lanes])
        buffers.append(hb)
        by_lanes[lanes] = (parts, len(o) - 1, len(b), w, A.collapse(w), GR.collapse_taxid_gi(w))
    yield ix, by_lanes
    for hb in buffers:
        hb.close()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("plain", [False, True], ids=["packed", "plain"])
def test_parts_across_segments_with_both_stages_filling(case, plain, lanes, monkeypatch):
    ix, by_lanes = case
    parts, n, n_bases, want, want_taxid, want_gi = by_lanes[lanes]
    monkeypatch.setenv("MTSV_ARENA_BASES", str(ARENA_BASES))
    if plain:
        monkeypatch.setenv("MTSV_H2D_PLAIN", "1")
    else:
        monkeypatch.delenv("MTSV_H2D_PLAIN", raising=False)
    b = M.Batch(ix, 0, 97, 1 << 14, lanes=1) if lanes == 1 else M.Batch(ix, 0, n, n_bases, lanes=2)
    for _ in range(2):                                  # assignments off: the hit stage alone, then from its last total
        b.run_host_parts(parts)
        assert b.stats()["n_lanes"] == lanes and b.stats()["n_reads"] == n
        assert_same_hits(b.download(), want)
    b.set_assignments(M.ASSIGN_WITH_HITS)               # both stages, 16-byte records
    for _ in range(2):
        b.run_host_parts(parts)
        a, _ms = b.download_assignments()
        assert A.as_triples(a) == want_taxid
        assert_same_hits(b.download(), want)
    b.set_assignments(M.ASSIGN_OFF)
    b.set_assignment_grain(M.GRAIN_TAXID_GI)            # both stages, 24-byte records: the assignment stage starts anew
    b.set_assignments(M.ASSIGN_WITH_HITS)
    for _ in range(2):
        b.run_host_parts(parts)
        a, _ms = b.download_assignments_gi()
        assert GR.as_tuples(a) == want_gi
        assert_same_hits(b.download(), want)
    assert b.stats()["n_lanes"] == lanes
    b.close()
