"""-m gpu: the seed stage by tiles.  k_thin_tiled takes T = 128 consecutive reads of a pass per workgroup (counts, read
offsets and the bit streams of the tile's byte span in LDS; the policy out of LDS; planes cut out of the streams at the
reads' bit offsets) and writes no seed_pre; k_expand_tiled forms a kept seed's offset inside its strand from the counts in
front of it, staged in LDS behind a halo of 16 slots.  Passes with max_ns <= 16 and reads up to 256 bases take this path,
the others (and every pass of a workspace created under MTSV_SEED_STAGE=legacy) k_thin and k_expand with seed_pre between
them; mtsv_batch_stats.n_seed_tile_passes says which.

Every batch is compared hit for hit with the CPU oracle and its work counters with the oracle's, through the C ABI, and is
also run on a legacy workspace whose hit array must be equal.  The cases: read counts at the tile's edges, resident
and as host batches on a workspace of two lanes whose ranges start inside a tile; reads at every byte offset modulo 64
with lengths on both sides of the plane words' edges and of the seed size; strands that hold seeds of 1, 2, 16, 17 and 80
hits side by side with dropped seeds in front of kept ones, on the three index layouts; parameter sets on both sides of
the tile's max_ns limit."""
import os
import random

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O
from test_read_planes import EDGES, RATE, ed_of, edge_reads, n_count, origin, with_n

pytestmark = pytest.mark.gpu

T = 128        # reads per workgroup of k_thin_tiled
MAX_NS = 16    # seed slots per strand the tile holds
COUNTS = [1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 8 * T + 3]
STRESS = dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5)  # test_gpu_parity's
UNIT = 1699    # distinct reads of the host batches
REPS = 40
WS_READS = REPS * UNIT // 2  # per lane: 33 980 reads, no multiple of T
PLANTS = (1, 2, 16, 17, 80)


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """helpers.tricky_db (tandem repeat: seeds of ~40 hits; conserved gene: 1..24) and five segments planted 1, 2, 16, 17
    and 80 times"""
    entries, gene, unit = helpers.tricky_db(seed=7)
    rng = random.Random(1212)
    segs = [helpers.rnd_seq(rng, 200) for _ in PLANTS]
    entries = entries + helpers.planted_db(rng, [], [(s, [(700 + 10 * k + c % 5, 90000 + 100 * k + c) for c in range(n)])
                                                    for k, (s, n) in enumerate(zip(segs, PLANTS))])
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "seed_stage.idx")
    ix.write(p)
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    texts = [bytes(c if c in b"ACGT" else 65 for c in t) for t in texts]
    return ix, O.Index.read(p), texts, segs, unit


@pytest.fixture(scope="module")
def unit(db):
    """1 699 reads of mixed lengths, one in four without a seed hit, and the oracle's word on them at default parameters"""
    ix, orc, texts, _, _ = db
    rng = random.Random(7100)
    reads = []
    while len(reads) < UNIT:
        L = rng.choice(EDGES[3:] + [150] * 8)
        reads += [helpers.rnd_seq(rng, L)] if len(reads) % 4 == 1 else edge_reads(rng, texts, L, 1)
    mp, op = both_params(edit_rate=RATE)
    b, o = helpers.reads_to_batch(reads)
    want, ctr = orc.bin_batch(b, o, op, threads=8)
    assert len(want) > 1000
    return reads, want, ctr


def workspaces(ix, n_reads, n_bases, **kw):
    """(the default workspace, one created under MTSV_SEED_STAGE=legacy)"""
    assert "MTSV_SEED_STAGE" not in os.environ
    new = M.Batch(ix, 0, n_reads, n_bases, **kw)
    os.environ["MTSV_SEED_STAGE"] = "legacy"
    try:
        old = M.Batch(ix, 0, n_reads, n_bases, **kw)
    finally:
        del os.environ["MTSV_SEED_STAGE"]
    return new, old


COUNTERS = ("n_seed_hits", "n_candidates", "n_verified", "window_bytes", "n_hits")


def check(got, st, want, ctr, what, cut=False):
    """cut: max_assignments is set.  The reference's loop stops at the strand's last assignment; the device verifies the
    first candidates of a strand's TaxIDs side by side and applies max_assignments afterwards, in k_resolve (DESIGN.md
    section 3), so n_verified and window_bytes are then bounded below by the oracle's, not equal to them -- with any seed
    stage (the stress set on this file's ladder batch: 149 and 29 549 against the oracle's 148 and 29 230, on a default and
    on a legacy workspace alike).  Such a batch is run a second time without the cut, where all five counters are the oracle's."""
    assert_same_hits(got, want)
    assert (st["n_seed_hits"], st["n_candidates"], st["n_hits"]) == (ctr["H"], ctr["n_cand"], len(want)), what
    if cut:
        assert st["n_verified"] >= ctr["n_sw"] and st["window_bytes"] >= ctr["W"], what
    else:
        assert (st["n_verified"], st["window_bytes"]) == (ctr["n_sw"], ctr["W"]), what


def same_fields(a, b):
    """the two hit arrays are equal, field by field (the struct's padding bytes are not part of a hit)"""
    assert len(a) == len(b)
    for f in helpers.FIELDS:
        assert np.array_equal(a[f], b[f]), f


def check_path(st, tiles, what):
    """tiles: 'all', 'none' or 'some' of the run's passes took the tile path"""
    n, p = st["n_seed_tile_passes"], st["n_passes"]
    assert p >= 1, what
    if tiles == "all":
        assert n == p, (what, n, p)
    elif tiles == "none":
        assert n == 0, (what, n, p)
    else:
        assert 0 < n < p, (what, n, p)


def run_resident(db, reads, over, tiles="all", min_hits=1, modes=(0,), **kw):
    """the batch resident on a default and on a legacy workspace: oracle, counters, path taken, new == legacy"""
    ix, orc = db[0], db[1]
    bases, off = helpers.reads_to_batch(reads)
    mp, op = both_params(**over)
    want, ctr = orc.bin_batch(bases, off, op, threads=8)
    assert len(want) >= min_hits, len(want)
    new, old = workspaces(ix, max(len(reads), 1), max(len(bases), 1), **kw)
    try:
        for mode in modes:
            outs = []
            for name, b, t in (("tiles", new, tiles), ("legacy", old, "none")):
                b.set_verify_mode(mode)
                b.upload(bases, off)
                b.run(mp)
                got, st = b.download(), b.stats()
                check(got, st, want, ctr, (name, mode), cut=over.get("max_assignments") is not None)
                check_path(st, t, (name, mode))
                outs.append((got, st))
            same_fields(outs[0][0], outs[1][0])
            assert [outs[0][1][k] for k in COUNTERS] == [outs[1][1][k] for k in COUNTERS], mode
    finally:
        new.close()
        old.close()
    return want, outs[0][1]  # (the default workspace's stats)


# ---- 1. tile edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_read_counts_at_the_tile_edges_resident(db, unit, count):
    """the last workgroup of k_thin_tiled holds 1 .. T reads, and k_expand_tiled's last wavefront a part of a strand"""
    db[0].to_device(0)
    reads = unit[0][:count]
    run_resident(db, reads, dict(edit_rate=RATE), min_hits=0 if count < 3 else 1, modes=(0, 1))


def test_passes_that_start_inside_a_tile_resident(db, unit):
    """a hit workspace too small for the batch: the pass is halved until it fits, so passes begin at read indices
    (r0) that are no multiple of T and their tiles at any byte offset"""
    db[0].to_device(0)
    reads = unit[0][:8 * T + 3]
    _, st = run_resident(db, reads, dict(edit_rate=RATE), max_hits_ws=3000)
    assert st["n_passes"] >= 4, st["n_passes"]


@pytest.mark.parametrize("count", COUNTS)
def test_read_counts_at_the_tile_edges_host_two_lanes(db, unit, count):
    """run_host of 40 x 1 699 + count reads on a workspace of two lanes of 33 980 reads: the ranges begin at read indices
    that are no multiple of T and at byte offsets that are no multiple of 64 (neighbouring ranges unpack into the same
    64-byte group on two streams), and the last range holds the count's tail"""
    ix, orc, _, _, _ = db
    ix.to_device(0)
    ureads, uwant, uctr = unit
    mp, op = both_params(edit_rate=RATE)
    tb, to = helpers.reads_to_batch(ureads[:count])
    twant, tctr = orc.bin_batch(tb, to, op, threads=8)
    parts = []
    for k in range(REPS):
        h = uwant.copy()
        h["read"] += k * UNIT
        parts.append(h)
    twant = twant.copy()
    twant["read"] += REPS * UNIT
    want = np.concatenate(parts + [twant])
    ctr = {k: v * REPS + tctr[k] for k, v in uctr.items()}
    bases, off = helpers.reads_to_batch(ureads * REPS + ureads[:count])
    assert WS_READS % T and {int(o) % 64 for o in off[WS_READS::WS_READS]} != {0}
    new, old = workspaces(ix, 2 * WS_READS, 2 * WS_READS * 170, lanes=2)
    try:
        outs = []
        for name, b, tiles in (("tiles", new, "all"), ("legacy", old, "none")):
            b.run_host(bases, off, mp)
            got, st = b.download(), b.stats()
            check(got, st, want, ctr, name)
            check_path(st, tiles, name)
            assert st["n_lanes"] == 2 and st["n_passes"] >= 3, (name, st["n_lanes"], st["n_passes"])
            outs.append((got, st))
        same_fields(outs[0][0], outs[1][0])
        assert [outs[0][1][k] for k in COUNTERS] == [outs[1][1][k] for k in COUNTERS]
    finally:
        new.close()
        old.close()


# ---- 2. bit offsets ------------------------------------------------------------------------------------------------------
def test_reads_at_every_byte_offset_and_word_edge(db):
    """a few hundred reads of every length of EDGES and of 0, 1, 17, 18 and 19 bases (below, at and above the seed size),
    shuffled: reads start at every byte offset modulo 64, the pass's plane_words exceeds most reads' own word counts,
    N sits at the reads' first and last bases and on both sides of positions 32j, reads with exactly ED and ED + 1 N
    (the hopeless flag's edge) and random reads without a seed hit lie between them"""
    ix, orc, texts, _, _ = db
    ix.to_device(0)
    rng = random.Random(7200)
    tagged = []  # (read, it is random sequence)
    for L in EDGES:
        tagged += [(r, False) for r in edge_reads(rng, texts, L, 12)]
        ed = ed_of(L)
        for k in (ed, ed + 1):
            for at in (rng.sample(range(L), k), range(k), range(L - k, L)):
                r = with_n(origin(rng, texts, L)[:L], at)
                assert n_count(r) == k
                tagged.append((r if rng.random() < 0.5 else helpers.revcomp(r), False))
        tagged += [(helpers.rnd_seq(rng, L), True) for _ in range(4)]
    for L in (0, 1, 17, 18, 19):
        tagged += [(origin(rng, texts, L)[:L], False) for _ in range(4)]
    for order in range(100):  # the first shuffle that puts a read at every byte offset modulo 64
        random.Random(7250 + order).shuffle(tagged)
        starts = np.cumsum([0] + [len(r) for r, _ in tagged])[:-1]
        if {int(s) % 64 for s in starts} == set(range(64)):
            break
    reads = [r for r, _ in tagged]
    assert {int(s) % 64 for s in starts} == set(range(64))
    assert 300 < len(reads) < 1000 and max(map(len, reads)) == 253
    want, _ = run_resident(db, reads, dict(edit_rate=RATE), min_hits=len(reads) // 3, modes=(0, 1))
    hit_reads = set(want["read"].tolist())
    for i, r in enumerate(reads):
        if n_count(r) > ed_of(len(r)) or len(r) < 18 or tagged[i][1]:
            assert i not in hit_reads
    between = [i for i in range(1, len(reads) - 1) if tagged[i][1] and i - 1 in hit_reads and i + 1 in hit_reads]
    assert len(between) >= 10, len(between)


# ---- 3. prefix sums in k_expand_tiled ------------------------------------------------------------------------------------
def ladder_reads(db, rng):
    """reads of 150 bases that are 30-base pieces of the planted segments in a row (copies: 1, 2, 16, 17, 80, in every
    rotation and on both strands): the seeds at read offsets 0, 30, ... lie inside a piece and have that many hits, those
    at 15, 45, ... straddle two pieces and have none.  With them reads from the tandem repeat (every seed ~40 hits), from
    the database at large, and random ones"""
    _, _, texts, segs, rep_unit = db
    reads = []
    for rot in range(len(segs)):
        for st in (0, 7, 50):
            order = segs[rot:] + segs[:rot]
            r = b"".join(s[st + 30 * k:st + 30 * k + 30] for k, s in enumerate(order))
            reads += [r, helpers.revcomp(r), helpers.substitute(rng, r, 3)]
    rep = rep_unit * 5
    for _ in range(20):
        st = rng.randrange(0, len(rep) - 150)
        reads.append(helpers.mutate(rng, rep[st:st + 150], rng.randrange(0, 6), b"ACGT"))
    for _ in range(30):
        reads += edge_reads(rng, texts, rng.choice([97, 150, 253]), 1)
        reads.append(helpers.rnd_seq(rng, 150))
    rng.shuffle(reads)
    return reads


@pytest.mark.parametrize("flags", [0, 2, 1], ids=["kmer_table", "no_table", "sampled_sa"])
@pytest.mark.parametrize("pname,over", [("default", {}), ("stress", STRESS), ("tune1", dict(tune_max_hits=1))])
def test_offsets_of_kept_seeds_behind_dropped_and_heavy_ones(db, pname, over, flags):
    """one strand holds seeds of 1, 2, 16, 17 and 80 hits side by side (a lane's own loop, its edge at 16, the wavefront's
    walk).  Default parameters keep them all; the stress set drops the heavy ones in front of kept ones and doubles the
    interval behind a seed of more than two hits; tune_max_hits = 1 doubles it behind the seed of two.  With the k-mer
    table singletons arrive as kSeedAtPos, without it as intervals of one row; with the sampled SA alone the rows go
    through hit_row and k_locate"""
    ix = db[0]
    ix.to_device(0, flags)
    try:
        reads = ladder_reads(db, random.Random(7300))
        want, st = run_resident(db, reads, over, min_hits=20)  # (the stress set returns one hit per read at most)
        if over.get("max_assignments") is not None:  # the same seed policy without the cut: every counter is the oracle's
            run_resident(db, reads, dict(over, max_assignments=None), min_hits=20)
        if pname == "default":
            assert st["n_seed_hits"] > 5000, st["n_seed_hits"]
    finally:
        ix.to_device(0)


# ---- 4. the fallback's edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval,tiles", [(15, "all"), (14, "none")])
def test_max_ns_on_both_sides_of_the_tile_limit(db, unit, interval, tiles):
    """reads up to 253 bases, seeds of 18: an interval of 15 gives max_ns = 16, the limit; 14 gives 17 and k_thin"""
    db[0].to_device(0)
    reads = [r for r in unit[0][:600]]
    assert max(map(len, reads)) == 253 and (253 - 18) // interval + 1 == (MAX_NS if tiles == "all" else MAX_NS + 1)
    run_resident(db, reads, dict(edit_rate=RATE, seed_interval=interval), tiles=tiles, min_hits=100)


def test_dense_seeds_keep_the_legacy_kernels(db, unit):
    """test_gpu_parity's dense set: seeds of 10 every 3 bases, max_ns = 82"""
    db[0].to_device(0)
    run_resident(db, unit[0][:300], dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30), tiles="none", min_hits=100)


def test_a_long_read_among_short_ones(db, unit):
    """a read above 256 bases runs in a pass of its own through the tiled verify kernel, with max_ns = 26: that pass keeps
    k_thin and k_expand, the passes in front of it and behind it go by tiles"""
    _, _, texts, _, _ = db
    db[0].to_device(0)
    rng = random.Random(7400)
    reads = unit[0][:T + 5] + [origin(rng, texts, 400)[:400]] + unit[0][T + 5:2 * T + 9]
    want, st = run_resident(db, reads, dict(edit_rate=RATE), tiles="some", min_hits=100)
    assert st["n_passes"] == 3 and st["n_seed_tile_passes"] == 2
    assert T + 5 in set(want["read"].tolist())
