"""-m gpu tests of the wide grains of the assignments (k_collapse.hip under MTSV_GRAIN_LONG and MTSV_GRAIN_TAXID_GI,
mtsv_batch_set_assignment_grain / mtsv_batch_download_assignments_gi): per read one 24-byte record per distinct
(tax_id, gi, offset) with the smallest edit, or per distinct (tax_id, gi) with the smallest (edit, offset), reduced on the
device.  The expected records always come from the CPU oracle's hits through the Python restatement (grain_ref.py), never
from the device's own hits; what the hits must hold for a test to mean something (grain_cases.census) is asserted on the
oracle's hits before the device is looked at."""
import collections
import os
import random
import re
import subprocess

import numpy as np
import pytest

import assign_ref as A
import grain_cases as G
import grain_ref as GR
import helpers
import mtsv_tools_amd as M
import taxa_report_ref as R
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COLLAPSE = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")

STRESS = dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5)
PARAM_SETS = {
    "default": {},
    "stress": STRESS,
    "dense": dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30),
    "loose": dict(edit_rate=0.3, max_candidates=40),
}
GRAINS = {"taxid_gi": (M.GRAIN_TAXID_GI, GR.collapse_taxid_gi, " [grain taxid-gi]"), "long": (M.GRAIN_LONG, GR.collapse_long, " [grain long]")}
TIERS = re.compile(r"\[collapse\] (\w+): (\d+) launches, [0-9.]+ ms, (\d+) hits -> (\d+) assignments; reads by tier: lane (\d+), wavefront (\d+), "
                   r"lds (\d+), global (\d+) \(tiers end at (\d+) / (\d+) / (\d+) hits\)([^\n]*)\n")
LDS_KEYS_WIDE = 2048


def both_params(**over):
    return M.default_params(**over), O.default_params(**{("seed_gap" if k == "seed_interval" else k): v for k, v in over.items()})


def oracle_hits(orc, bases, off, op=None):
    want, _ = orc.bin_batch(bases, off, op or O.default_params(), threads=8)
    return want


def got_records(b):
    a, ms = b.download_assignments_gi()
    assert ms >= 0
    return GR.as_tuples(a)


def resident(ix, bases, off, grain, mp=None, mode=M.ASSIGN_WITH_HITS, vmode=None, **kw):
    """upload + run with the assignments on in `grain`; returns (records, hits, stats)"""
    b = M.Batch(ix, 0, max(len(off) - 1, 1), max(len(bases), 1), **kw)
    if vmode is not None:
        b.set_verify_mode(vmode)
    b.set_assignment_grain(grain)
    b.set_assignments(mode)
    b.upload(bases, off)
    b.run(mp)
    out = got_records(b), b.download(), b.stats()
    b.close()
    return out


def built(entries, tmp, name):
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp / f"{name}.idx")
    ix.write(p)
    ix.to_device(0)
    return ix, O.Index.read(p)


def expected_tiers(hits, n_reads, lane_max, wave_max, lds_max):
    """reads by tier (lane, wavefront, lds, global) from the oracle's per-read hit counts"""
    per_read = np.bincount(hits["read"].astype(np.int64), minlength=n_reads)
    lane = int(((per_read >= 1) & (per_read <= lane_max)).sum())
    wave = int(((per_read > lane_max) & (per_read <= wave_max)).sum())
    rest = per_read[(per_read > lane_max) & (per_read > wave_max)]
    return lane, wave, int((rest <= lds_max).sum()), int((rest > lds_max).sum())


def traced_tiers(err, suffix, what="run"):
    m = [t for t in TIERS.findall(err) if t[0] == what]
    assert len(m) == 1, err
    assert m[0][11] == suffix, m[0]
    return tuple(int(x) for x in m[0][4:8]), tuple(int(x) for x in m[0][8:11]), int(m[0][2]), int(m[0][3])


def set_edges(monkeypatch, env):
    for k in ("LANE_MAX", "WAVE_MAX", "LDS_MAX"):
        monkeypatch.delenv("MTSV_COLLAPSE_" + k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("MTSV_COLLAPSE_" + k, str(v))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    ix = M.MGIndex.build_fasta(os.path.join(GOLD, "e2e_db.fasta"), threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "golden.idx")
    ix.write(p)
    ix.to_device(0)
    reads = [l.rstrip("\n").encode("latin-1") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    return ix, O.Index.read(p), reads


@pytest.fixture(scope="module")
def tricky(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix, orc = built(entries, tmp_path_factory.mktemp("idx"), "tricky")
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=40, lengths=(150, 320))
    return ix, orc, reads, entries, gene, unit


@pytest.fixture(scope="module")
def chunks(tmp_path_factory):
    """chunk A and chunk B of the case database on the device, 40 reads of the segment (160 hits each in A), 10 across the
    palindrome, 60 of one hit; the oracle's hits per chunk"""
    first, second, seg, half, rng = G.database()
    d = tmp_path_factory.mktemp("idx")
    (ix1, orc1), (ix2, orc2) = built(first, d, "a"), built(second, d, "b")
    reads = G.reads(rng, seg, half, first)
    random.Random(4).shuffle(reads)
    bases, off = helpers.reads_to_batch(reads)
    parts = [oracle_hits(o, bases, off) for o in (orc1, orc2)]
    return (ix1, ix2), bases, off, parts, len(reads)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    ix = M.MGIndex.synth(seed=5, n_taxa=24, gis_per_taxon=2, seq_len=20000)
    p = str(tmp_path_factory.mktemp("idx") / "synth.idx")
    ix.write(p)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=9, n_reads=65_536, read_len=150)
    want = oracle_hits(O.Index.read(p), bases, off)
    return ix, bases, off, want, GR.collapse_long(want)


# ---- 1. golden database ----

def test_golden_database_gives_the_recorded_long_lines(golden):
    ix, orc, reads = golden
    bases, off = helpers.reads_to_batch(reads)
    ids = [f"r{i}" for i in range(len(reads))]
    for name, over in (("default", {}), ("stress", STRESS)):
        mp, op = both_params(**over)
        want = GR.collapse_long(oracle_hits(orc, bases, off, op))
        lines = sorted(open(os.path.join(GOLD, f"e2e_{name}_long.results")).read().splitlines())
        assert sorted(GR.text(want, ids).splitlines()) == lines
        for mode in (M.ASSIGN_WITH_HITS, M.ASSIGN_ONLY):
            got, hits, _ = resident(ix, bases, off, M.GRAIN_LONG, mp, mode)
            assert got == want
            assert sorted(M.format_assignments_gi(GR.as_array(got, M.ASSIGN_GI_DTYPE), ids).splitlines()) == lines
        b = M.Batch(ix, 0, len(reads), len(bases))
        b.set_assignment_grain(M.GRAIN_LONG)
        b.set_assignments(M.ASSIGN_ONLY)
        b.run_host(bases, off, mp)
        a, _ = b.download_assignments_gi()
        b.close()
        assert sorted(M.format_assignments_gi(a, ids).splitlines()) == lines


# ---- 2. tricky database ----

@pytest.mark.parametrize("vmode", [0, 1])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("gname", list(GRAINS))
def test_adversarial_database_parameter_sets_and_verify_orders(tricky, gname, pname, vmode):
    ix, orc, reads = tricky[:3]
    grain, restate, _ = GRAINS[gname]
    mp, op = both_params(**PARAM_SETS[pname])
    bases, off = helpers.reads_to_batch(reads)
    hits = oracle_hits(orc, bases, off, op)
    want = restate(hits)
    assert len(want) > 50 and any(t > 1 << 31 for _, t, _, _, _ in want)
    got, dev_hits, st = resident(ix, bases, off, grain, mp, M.ASSIGN_WITH_HITS, vmode)
    assert got == want
    assert_same_hits(dev_hits, hits)
    got, dev_hits, st = resident(ix, bases, off, grain, mp, M.ASSIGN_ONLY, vmode)
    assert got == want
    assert len(dev_hits) == 0 and st["n_hits"] == len(hits)


# ---- 3. tiers at their edges ----

@pytest.mark.parametrize("gname", list(GRAINS))
def test_tiers_at_their_edges(chunks, gname, monkeypatch, capfd):
    (ix, _), bases, off, parts, n = chunks
    hits = parts[0]
    grain, restate, suffix = GRAINS[gname]
    want = restate(hits)
    per_read = collections.Counter(hits["read"].tolist())
    h = max(per_read.values())
    n_big = sum(c > 64 for c in per_read.values())
    # (one index never returns one (tax_id, gi, offset) with two edits: that comparison is the collector test's; the
    #  palindrome gives the long key twice with equal edits)
    c = G.census(hits)
    assert c["tax31"] and c["gi31"] and c["by_offset"] and c["offset_decides"] and c["winner_later"] and c["same_edit"], c
    assert 128 < h <= 256 and n_big >= 30 and sum(v == 1 for v in per_read.values()) > 40 and len(want) < len(hits)
    monkeypatch.setenv("MTSV_TRACE", "1")

    def run(env):
        set_edges(monkeypatch, env)
        capfd.readouterr()
        got, _, _ = resident(ix, bases, off, grain, mode=M.ASSIGN_ONLY)
        counts, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err, suffix)
        assert got == want, env
        assert (n_hits, n_assign) == (len(hits), len(want))
        lane_max, wave_max = min(int(env.get("LANE_MAX", 16)), 16), min(int(env.get("WAVE_MAX", 64)), 64)
        lds_max = min(int(env.get("LDS_MAX", LDS_KEYS_WIDE)), LDS_KEYS_WIDE)   # the wide grains' LDS tier ends at 2048 keys
        lds_max = 1 << (lds_max.bit_length() - 1)                              # a power of two: anything else is rounded down
        assert edges == (lane_max, wave_max, lds_max), env                     # the trace reports the effective edges
        assert counts == expected_tiers(hits, n, *edges), env
        return counts

    c = run({})
    assert c[0] > 40 and c[1] == 0 and c[2] == n_big and c[3] == 0   # the LDS tier takes the heavy reads
    c = run({"LDS_MAX": 64})
    assert c[2] == 0 and c[3] == n_big                               # ... now the global tier does
    for lm in (1, 4):
        c = run({"LANE_MAX": lm})
        assert c[0] > 40 and c[2] == n_big
    c = run({"LDS_MAX": 300})                                        # rounded down to 256: still the LDS tier
    assert c[2] == n_big and c[3] == 0
    c = run({"LDS_MAX": 200, "WAVE_MAX": 8, "LANE_MAX": 2})          # rounded down to 128: the global tier
    assert c[2] == 0 and c[3] == n_big
    c = run({"LDS_MAX": 4096})                                       # clamped, and reported as clamped
    assert c[2] == n_big and c[3] == 0


@pytest.mark.parametrize("gname", list(GRAINS))
def test_wavefront_tier_with_more_than_32_keys(gname, tmp_path, monkeypatch, capfd):
    """the case database on 30 sequences: 20 distinct TaxIDs (ten numbers, each with and without bit 31), met once per strand,
    so a read of the segment carries 40 hits -- the wavefront tier with keys in the upper lanes, and its edge at that count.
    (Thirty sequences and not twenty: a strand returns a TaxID once, so twenty sequences give 28 hits, below the 33..64 the
    case is for.)"""
    first, _, seg, half, rng = G.database(n_seq=30)
    ix, orc = built(first, tmp_path, "wave")
    reads = G.reads(rng, seg, half, first, n_seg=30, n_pal=6, n_bg=30)
    random.Random(8).shuffle(reads)
    bases, off = helpers.reads_to_batch(reads)
    hits = oracle_hits(orc, bases, off)
    grain, restate, suffix = GRAINS[gname]
    want = restate(hits)
    per_read = collections.Counter(hits["read"].tolist())
    h = max(per_read.values())
    n_big = sum(c == h for c in per_read.values())
    c = G.census(hits)
    assert 32 < h < 64 and n_big >= 25 and len(want) < len(hits), (h, n_big)
    assert c["tax31"] and c["gi31"] and c["offset_decides"] and c["winner_later"], c
    monkeypatch.setenv("MTSV_TRACE", "1")
    n_two = sum(c == 2 for c in per_read.values())             # (the palindrome's reads: a lane's, unless a lane takes one hit only)
    assert n_two and set(per_read.values()) == {1, 2, h}
    for env, tier, n_tier in (({}, 1, n_big), ({"WAVE_MAX": h - 1}, 2, n_big), ({"WAVE_MAX": h}, 1, n_big), ({"WAVE_MAX": h + 1}, 1, n_big),
                              ({"WAVE_MAX": h - 1, "LDS_MAX": 32}, 3, n_big), ({"LANE_MAX": 1, "WAVE_MAX": 64}, 1, n_big + n_two)):
        set_edges(monkeypatch, env)
        capfd.readouterr()
        got, _, _ = resident(ix, bases, off, grain, mode=M.ASSIGN_ONLY)
        counts, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err, suffix)
        assert got == want, env
        assert counts == expected_tiers(hits, len(reads), *edges), env
        assert counts[tier] == n_tier, env


# ---- 4. collector ----

def test_collector_records_equal_mtsv_collapse_on_the_chunk_long_files(chunks, tmp_path):
    (ix1, ix2), bases, off, parts, n = chunks
    both = np.concatenate(parts)
    c = G.census(both)
    # every comparison the keys can be decided by, a winner that is not the first hit, a group of four
    assert c["tax31"] and c["gi31"] and c["offset_decides"] and c["by_edit"] and c["edit_later"] and c["winner_later"], c
    assert c["group_max"] == 4 and c["gis_max"] == 3, c
    ids = [f"read{i}" for i in range(n)]
    files = []
    for k, p in enumerate(parts):
        f = tmp_path / f"chunk{k}.long"
        f.write_text(M.format_results(p, ids, long_format=True))
        files.append(str(f))
    out = tmp_path / "collapsed.txt"
    r = subprocess.run([COLLAPSE, "--mode", "taxid-gi", "-o", str(out), *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    srcs = [M.Batch(ix, 0, n, len(bases)) for ix in (ix1, ix2)]
    srcs[0].upload(bases, off)
    srcs[1].copy_reads(srcs[0])
    for s in srcs:
        s.run()
    want = {g: GRAINS[g][1](both) for g in GRAINS}
    assert len(want["taxid_gi"]) < len(want["long"]) < len(both)
    dst = M.Batch(ix1, 0, 64, 1 << 12)
    for gname, (grain, restate, _) in GRAINS.items():
        dst.set_assignments(M.ASSIGN_OFF)
        dst.set_assignment_grain(grain)
        dst.set_assignments(M.ASSIGN_WITH_HITS)
        dst.merge_runs(srcs)
        assert got_records(dst) == want[gname]
        assert len(dst.download()) == len(both)
    # (the collector is in GRAIN_LONG now) a refused merge leaves its records readable
    srcs[1].set_match_flags(M.MATCH_ONLY)
    with pytest.raises(M.MtsvError) as e:
        dst.merge_runs(srcs)
    assert e.value.code == _lib.E_ARG
    assert got_records(dst) == want["long"]
    srcs[1].set_match_flags(M.MATCH_OFF)
    # taxid-gi over the chunks is what mtsv-collapse --mode taxid-gi makes of the chunks' long files
    dst.set_assignments(M.ASSIGN_OFF)
    dst.set_assignment_grain(M.GRAIN_TAXID_GI)
    dst.set_assignments(M.ASSIGN_ONLY)
    dst.merge_runs(srcs)
    a, _ = dst.download_assignments_gi()
    assert sorted(M.format_assignments_gi(a, ids).splitlines()) == sorted(out.read_text().splitlines())
    assert len(dst.download()) == 0 and dst.stats()["n_hits"] == len(both)
    # a merge of one source is that run
    dst.merge_runs(srcs[:1])
    assert got_records(dst) == GR.collapse_taxid_gi(parts[0])
    assert len(dst.download()) == 0 and dst.stats()["n_hits"] == len(parts[0])
    for b in srcs + [dst]:
        b.close()


def merged(srcs, dst, grain, mode=M.ASSIGN_ONLY):
    """the collector's records of `grain` from a merge of srcs (the tier edges are read as the assignments are switched on)"""
    dst.set_assignments(M.ASSIGN_OFF)
    dst.set_assignment_grain(grain)
    dst.set_assignments(mode)
    dst.merge_runs(srcs)
    return got_records(dst)


@pytest.mark.parametrize("gname", list(GRAINS))
def test_collector_hits_through_every_tier(chunks, gname, tmp_path, monkeypatch, capfd):
    """only merged hits hold one (tax_id, gi, offset) with two edits and groups of four: those comparisons through the global
    tier and with the lane tier's edge moved (chunks A and B: reads of 280 hits), and, on the 24-sequence variant whose merged
    reads carry 56 hits, through the wavefront tier and the lane-per-read tier's neighbours"""
    grain, restate, suffix = GRAINS[gname]
    monkeypatch.setenv("MTSV_TRACE", "1")

    def through(ixs, bases, off, parts, n, cases):
        both = np.concatenate(parts)
        c = G.census(both)
        assert c["tax31"] and c["gi31"] and c["offset_decides"] and c["by_edit"] and c["edit_later"] and c["winner_later"], c
        assert c["group_max"] == 4, c
        want = restate(both)
        srcs = [M.Batch(ix, 0, n, len(bases)) for ix in ixs]
        srcs[0].upload(bases, off)
        srcs[1].copy_reads(srcs[0])
        for b in srcs:
            b.run()
        dst = M.Batch(ixs[0], 0, 64, 1 << 12)
        n_big = int((np.bincount(both["read"].astype(np.int64), minlength=n) > 16).sum())
        for env, tier in cases:
            set_edges(monkeypatch, env)
            capfd.readouterr()
            got = merged(srcs, dst, grain)
            counts, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err, suffix, "merge")
            assert got == want, env
            assert (n_hits, n_assign) == (len(both), len(want))
            assert counts == expected_tiers(both, n, *edges), env
            assert counts[tier] == n_big > 0, env
        for b in srcs + [dst]:
            b.close()

    ixs, bases, off, parts, n = chunks
    assert max(np.bincount(np.concatenate(parts)["read"].astype(np.int64))) > 256
    through(ixs, bases, off, parts, n, (({}, 2), ({"LDS_MAX": 64}, 3), ({"LDS_MAX": 256}, 3), ({"LANE_MAX": 1, "LDS_MAX": 512}, 2)))
    first, second, seg, half, rng = G.database(n_seq=24)
    small = (built(first, tmp_path, "a24"), built(second, tmp_path, "b24"))
    reads = G.reads(rng, seg, half, first, n_seg=20, n_pal=4, n_bg=20)
    random.Random(5).shuffle(reads)
    sb, so = helpers.reads_to_batch(reads)
    sparts = [oracle_hits(o, sb, so) for _, o in small]
    h = int(max(np.bincount(np.concatenate(sparts)["read"].astype(np.int64))))
    assert 32 < h <= 64
    through([ix for ix, _ in small], sb, so, sparts, len(reads),
            (({}, 1), ({"WAVE_MAX": h}, 1), ({"WAVE_MAX": h - 1}, 2), ({"WAVE_MAX": h - 1, "LDS_MAX": 32}, 3), ({"LANE_MAX": 4}, 1)))


# ---- 5. how the reads arrive ----

def test_result_does_not_depend_on_how_the_reads_reach_the_device(synth):
    ix, bases, off, hits, want = synth
    n = len(off) - 1
    assert n == 65_536 and len(want) > 0.8 * n
    b = M.Batch(ix, 0, n, len(bases), lanes=2)
    b.set_assignment_grain(M.GRAIN_LONG)
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.run_host(bases, off)
    assert b.stats()["n_lanes"] == 2
    assert got_records(b) == want
    assert_same_hits(b.download(), hits)
    b.set_assignments(M.ASSIGN_ONLY)
    b.run_host(bases, off)
    assert got_records(b) == want
    assert len(b.download()) == 0 and b.stats()["n_hits"] == len(hits)
    h = 1000                                                # a second, shorter run replaces the first's records
    b.run_host(bases[: int(off[h])], off[: h + 1])
    assert got_records(b) == [t for t in want if t[0] < h]
    cuts = [0, 7, 7, 20_001, 20_002, 47_777, n]             # uneven pieces, an empty one among them
    parts = [(bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a]) for a, c in zip(cuts, cuts[1:])]
    b.run_host_parts(parts)
    assert got_records(b) == want
    assert got_records(b) == want                           # a download does not consume them
    # the other wide grain on the same workspace: off, the grain, on again
    b.set_assignments(M.ASSIGN_OFF)
    b.set_assignment_grain(M.GRAIN_TAXID_GI)
    b.set_assignments(M.ASSIGN_ONLY)
    b.run_host(bases, off)
    assert got_records(b) == GR.collapse_taxid_gi(hits)
    b.close()
    # a workspace so small that the batch takes many passes
    b = M.Batch(ix, 0, 3000, 3000 * 150)
    b.set_assignment_grain(M.GRAIN_LONG)
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.run_host(bases, off)
    assert b.stats()["n_passes"] >= 20
    assert got_records(b) == want
    assert_same_hits(b.download(), hits)
    b.close()


# ---- 6. a pass run again contributes once ----

def test_passes_that_are_run_again_contribute_once(tricky):
    ix, orc, reads = tricky[:3]
    reads = [r for r in reads if len(r) <= 253]
    mp, op = both_params(seed_size=11, seed_interval=4, max_hits=100000, tune_max_hits=100000, min_seed=0.1)
    bases, off = helpers.reads_to_batch(reads)
    want = GR.collapse_long(oracle_hits(orc, bases, off, op))
    got, _, st = resident(ix, bases, off, M.GRAIN_LONG, mp, max_hits_ws=64)
    assert st["n_passes"] > 100
    assert got == want


# ---- 7. behind a filter ----

def test_records_behind_a_filter_carry_the_callers_read_numbers(tricky, tmp_path):
    ix_d, orc_d, reads, entries = tricky[:4]
    rng = random.Random(77)
    own = [(700000 + k, 90000 + k, helpers.rnd_seq(rng, 2500)) for k in range(3)]
    ix_f, orc_f = built(entries[::3] + own, tmp_path, "filter")
    bases, off = helpers.reads_to_batch(reads)
    n = len(reads)
    in_f = np.zeros(n, dtype=bool)
    in_f[oracle_hits(orc_f, bases, off)["read"].astype(np.int64)] = True
    survivors = np.nonzero(~in_f)[0]
    assert 0 < len(survivors) < n
    sb, so = helpers.reads_to_batch([reads[i] for i in survivors])
    want_hits = oracle_hits(orc_d, sb, so)
    want_hits["read"] = survivors[want_hits["read"].astype(np.int64)]
    src = M.Batch(ix_f, 0, n, len(bases))
    src.set_match_flags(M.MATCH_ONLY)
    src.upload(bases, off)
    src.run()
    for gname, (grain, restate, _) in GRAINS.items():
        want = restate(want_hits)
        assert len(want) > 20 and any(r != i for i, r in enumerate(sorted({t[0] for t in want})))
        dst = M.Batch(ix_d, 0, n, len(bases))
        dst.set_assignment_grain(grain)
        dst.set_assignments(M.ASSIGN_WITH_HITS if gname == "long" else M.ASSIGN_ONLY)
        assert dst.take_reads(src, M.KEEP_UNMATCHED)[0] == len(survivors)
        dst.run()
        assert got_records(dst) == want
        if gname == "long":
            assert_same_hits(dst.download(), want_hits)
        dst.close()
    src.close()


# ---- 8. off is off, and refusals ----

def test_off_is_off_and_refusals(tricky):
    ix, orc, reads = tricky[:3]
    bases, off = helpers.reads_to_batch(reads)
    hits = oracle_hits(orc, bases, off)
    want = GR.collapse_long(hits)
    n = len(reads)
    plain = M.Batch(ix, 0, n, len(bases))
    plain.upload(bases, off)
    plain.run()
    on = M.Batch(ix, 0, n, len(bases))
    for bad in (-1, 3):                                      # a bad grain
        with pytest.raises(M.MtsvError) as e:
            on.set_assignment_grain(bad)
        assert e.value.code == _lib.E_ARG
    on.set_assignment_grain(M.GRAIN_LONG)
    with pytest.raises(M.MtsvError) as e:                    # the grain alone switches nothing on
        on.download_assignments_gi()
    assert e.value.code == _lib.E_ARG
    on.set_assignments(M.ASSIGN_WITH_HITS)
    on.upload(bases, off)
    on.run()
    assert_same_hits(plain.download(), hits)
    assert_same_hits(on.download(), hits)
    sp, so = plain.stats(), on.stats()
    assert {k: v for k, v in sp.items() if k.startswith("n_")} == {k: v for k, v in so.items() if k.startswith("n_")}
    assert got_records(on) == want
    # the grain while the assignments are on: refused, and nothing changes
    for g in (M.GRAIN_TAXID, M.GRAIN_TAXID_GI, M.GRAIN_LONG):
        with pytest.raises(M.MtsvError) as e:
            on.set_assignment_grain(g)
        assert e.value.code == _lib.E_ARG
    assert got_records(on) == want
    with pytest.raises(M.MtsvError) as e:                    # the 16-byte download under a wide grain
        on.download_assignments()
    assert e.value.code == _lib.E_ARG
    assert got_records(on) == want
    # MATCH_ONLY both ways
    plain.set_assignment_grain(M.GRAIN_TAXID_GI)
    plain.set_match_flags(M.MATCH_ONLY)
    with pytest.raises(M.MtsvError) as e:
        plain.set_assignments(M.ASSIGN_ONLY)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(M.MtsvError) as e:
        on.set_match_flags(M.MATCH_ONLY)
    assert e.value.code == _lib.E_ARG
    assert got_records(on) == want
    # off -> TAXID -> on: the 16-byte records, and the wide download refused
    on.set_assignments(M.ASSIGN_OFF)
    with pytest.raises(M.MtsvError) as e:
        on.download_assignments_gi()
    assert e.value.code == _lib.E_ARG
    on.set_assignment_grain(M.GRAIN_TAXID)
    on.set_assignments(M.ASSIGN_WITH_HITS)
    on.run()
    a, _ = on.download_assignments()
    assert A.as_triples(a) == A.collapse(hits)
    with pytest.raises(M.MtsvError) as e:
        on.download_assignments_gi()
    assert e.value.code == _lib.E_ARG
    # the report and the flags beside ASSIGN_ONLY in a wide grain
    on.set_assignments(M.ASSIGN_OFF)
    on.set_assignment_grain(M.GRAIN_TAXID_GI)
    on.set_assignments(M.ASSIGN_ONLY)
    on.set_taxa_report(True)
    on.set_match_flags(M.MATCH_WITH_HITS)
    on.run()
    assert got_records(on) == GR.collapse_taxid_gi(hits)
    assert len(on.download()) == 0
    rows, total, _ = on.taxa_report()
    stats, want_total = R.classify_hits(hits)
    assert (R.rows_dict(rows), total) == (stats, want_total)
    flags, n_matched = on.match_flags()
    present = np.zeros(n, dtype=bool)
    present[hits["read"].astype(np.int64)] = True
    assert np.array_equal(flags, present) and n_matched == int(present.sum())
    plain.close()
    on.close()


# ---- 9. command line ----

def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """the golden reads as FASTQ; the golden database whole, cut into two chunk indexes, and a filter of unrelated
    sequences (it removes no read: the lines stay the golden ones)"""
    d = tmp_path_factory.mktemp("grain_cli")
    reads = [l.rstrip("\n") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    fq = d / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i} desc\n{r}\n+\n{'I' * len(r)}\n")
    lines = open(os.path.join(GOLD, "e2e_db.fasta")).read().splitlines(keepends=True)
    starts = [i for i, l in enumerate(lines) if l.startswith(">")]
    mid = starts[len(starts) // 2]
    paths = {}
    for name, text in (("D", "".join(lines)), ("a", "".join(lines[:mid])), ("b", "".join(lines[mid:]))):
        fa = d / f"{name}.fasta"
        fa.write_text(text)
        paths[name] = str(d / f"{name}.idx")
        M.MGIndex.build_fasta(str(fa), threads=4).write(paths[name])
    rng = random.Random(12)
    paths["F"] = str(d / "F.idx")
    M.MGIndex.build([(900000 + k, 80000 + k, helpers.rnd_seq(rng, 2000)) for k in range(4)], threads=4).write(paths["F"])
    # (a database binned in two chunks is not the database binned whole: what --merge-on-gpu must write comes from the
    #  oracle on the two chunks, reduced over both)
    bases, off = helpers.reads_to_batch([r.encode("latin-1") for r in reads])
    parts = np.concatenate([oracle_hits(O.Index.read(paths[c]), bases, off) for c in ("a", "b")])
    chunk_lines = sorted(GR.text(GR.collapse_long(parts), [f"r{i}" for i in range(len(reads))]).splitlines())
    return fq, paths, chunk_lines


CLI_VARIANTS = {
    "plain": lambda p: ["-i", p["D"]],
    "two_workers": lambda p: ["-i", p["D"], "--devices", "0,0"],
    "batch_reads_9": lambda p: ["-i", p["D"], "--batch-reads", "9"],
    "filter_index": lambda p: ["-i", p["D"], "--filter-index", p["F"]],
    "merge_on_gpu": lambda p: ["-i", p["a"] + "," + p["b"], "--merge-on-gpu"],
}


@pytest.mark.parametrize("variant", list(CLI_VARIANTS))
def test_cli_writes_the_same_long_file_from_assignments(cli, variant, tmp_path):
    fq, paths, chunk_lines = cli
    want = sorted(open(os.path.join(GOLD, "e2e_default_long.results")).read().splitlines())
    if variant == "merge_on_gpu":
        assert chunk_lines != want and len(chunk_lines) == len(want)
        want = chunk_lines
    out = {}
    for setting in ("1", "0"):
        res = tmp_path / f"res{setting}.txt"
        r = run_binner("--fastq", fq, *CLI_VARIANTS[variant](paths), "-m", res, "--output-format", "long",
                       env={"MTSV_CLI_ASSIGN_LONG": setting, "MTSV_TRACE": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("[collapse]" in r.stderr) == (setting == "1")      # the setting is what decides which path wrote the file
        assert ("[grain long]" in r.stderr) == (setting == "1")
        out[setting] = res.read_bytes()
    assert out["1"] == out["0"]                                 # byte for byte: the lines are written in input order
    assert sorted(out["1"].decode().splitlines()) == want
