"""-m gpu tests of the assignments (k_collapse.hip, mtsv_batch_set_assignments / mtsv_batch_download_assignments): per read
one (tax_id, smallest edit) record per distinct TaxID, reduced on the device.  The expected records always come from the
CPU oracle's hits through the Python restatement (assign_ref.py), never from the device's own hits."""
import collections
import os
import random
import re
import subprocess

import numpy as np
import pytest

import assign_cases as K
import assign_ref as A
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

# (the parameter sets of the report test)
PARAM_SETS = {
    "default": {},
    "stress": dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5),
    "dense": dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30),
    "loose": dict(edit_rate=0.3, max_candidates=40),
    "one_assignment": dict(max_assignments=1),
    "two_assignments": dict(max_assignments=2),
    "two_candidates": dict(max_candidates=2),
}
TIERS = re.compile(r"\[collapse\] (\w+): (\d+) launches, [0-9.]+ ms, (\d+) hits -> (\d+) assignments; reads by tier: lane (\d+), wavefront (\d+), "
                   r"lds (\d+), global (\d+) \(tiers end at (\d+) / (\d+) / (\d+) hits\)")


def both_params(**over):
    return M.default_params(**over), O.default_params(**{("seed_gap" if k == "seed_interval" else k): v for k, v in over.items()})


def oracle_hits(orc, bases, off, op=None):
    want, _ = orc.bin_batch(bases, off, op or O.default_params(), threads=8)
    return want


def got_assignments(b):
    a, ms = b.download_assignments()
    assert ms >= 0
    return A.as_triples(a)


def resident(ix, bases, off, mp=None, mode=M.ASSIGN_WITH_HITS, vmode=None, **kw):
    """upload + run with the assignments on; returns (assignments, hits, stats)"""
    b = M.Batch(ix, 0, max(len(off) - 1, 1), max(len(bases), 1), **kw)
    if vmode is not None:
        b.set_verify_mode(vmode)
    b.set_assignments(mode)
    b.upload(bases, off)
    b.run(mp)
    out = got_assignments(b), b.download(), b.stats()
    b.close()
    return out


def built(entries, tmp, name):
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp / f"{name}.idx")
    ix.write(p)
    ix.to_device(0)
    return ix, O.Index.read(p)


def expected_tiers(hits, n_reads, lane_max=16, wave_max=64, lds_max=4096):
    """reads by tier (lane, wavefront, lds, global) from the oracle's per-read hit counts"""
    per_read = np.bincount(hits["read"].astype(np.int64), minlength=n_reads)
    lane = int(((per_read >= 1) & (per_read <= lane_max)).sum())
    wave = int(((per_read > lane_max) & (per_read <= wave_max)).sum())
    rest = per_read[(per_read > lane_max) & (per_read > wave_max)]
    return lane, wave, int((rest <= lds_max).sum()), int((rest > lds_max).sum())


def traced_tiers(err, what="run"):
    m = [t for t in TIERS.findall(err) if t[0] == what]
    assert len(m) == 1, err
    return tuple(int(x) for x in m[0][4:8]), tuple(int(x) for x in m[0][8:11]), int(m[0][2]), int(m[0][3])


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
def synth(tmp_path_factory):
    ix = M.MGIndex.synth(seed=5, n_taxa=24, gis_per_taxon=2, seq_len=20000)
    p = str(tmp_path_factory.mktemp("idx") / "synth.idx")
    ix.write(p)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=9, n_reads=100_000, read_len=150)
    want = oracle_hits(O.Index.read(p), bases, off)
    return ix, bases, off, want, A.collapse(want)


@pytest.fixture(scope="module")
def tiers(tmp_path_factory):
    """about 120 reads of 119..120 hits on 90 TaxIDs, mixed with ordinary reads of one hit"""
    entries, seg, rng = K.tier_db()
    ix, orc = built(entries, tmp_path_factory.mktemp("idx"), "tiers")
    reads = K.tier_reads(rng, seg, 120) + K.background_reads(rng, entries[:3], 200)
    random.Random(4).shuffle(reads)
    bases, off = helpers.reads_to_batch(reads)
    want = oracle_hits(orc, bases, off)
    return ix, bases, off, want, A.collapse(want), len(reads)


# ---- 1. golden database ----

def test_golden_database_gives_the_recorded_lines(golden):
    ix, orc, reads = golden
    bases, off = helpers.reads_to_batch(reads)
    want = A.collapse(oracle_hits(orc, bases, off))
    ids = [f"r{i}" for i in range(len(reads))]
    lines = sorted(open(os.path.join(GOLD, "e2e_default.results")).read().splitlines())
    assert sorted(A.text(want, ids).splitlines()) == lines
    for mode in (M.ASSIGN_WITH_HITS, M.ASSIGN_ONLY):
        got, hits, _ = resident(ix, bases, off, mode=mode)
        assert got == want
        assert sorted(M.format_assignments(A.as_array(got, M.ASSIGN_DTYPE), ids).splitlines()) == lines
    b = M.Batch(ix, 0, len(reads), len(bases))
    b.set_assignments(M.ASSIGN_ONLY)
    b.run_host(bases, off)
    a, _ = b.download_assignments()
    b.close()
    assert sorted(M.format_assignments(a, ids).splitlines()) == lines


# ---- 2. tricky database ----

@pytest.mark.parametrize("vmode", [0, 1])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_adversarial_database_parameter_sets_and_verify_orders(tricky, pname, vmode):
    ix, orc, reads = tricky[:3]
    mp, op = both_params(**PARAM_SETS[pname])
    bases, off = helpers.reads_to_batch(reads)
    assert max(map(len, reads)) > 256
    hits = oracle_hits(orc, bases, off, op)
    want = A.collapse(hits)
    assert len(want) > 50 and any(t > 1 << 31 for _, t, _ in want)
    got, dev_hits, st = resident(ix, bases, off, mp, M.ASSIGN_WITH_HITS, vmode)
    assert got == want
    assert_same_hits(dev_hits, hits)
    got, dev_hits, st = resident(ix, bases, off, mp, M.ASSIGN_ONLY, vmode)
    assert got == want
    assert len(dev_hits) == 0 and st["n_hits"] == len(hits)


# ---- 3. how the reads reach the device ----

def test_result_does_not_depend_on_how_the_reads_reach_the_device(synth):
    ix, bases, off, hits, want = synth
    n = len(off) - 1
    assert n >= 98304 and len(want) > 0.8 * n
    # (a) one resident upload + run: three lanes
    got, dev_hits, st = resident(ix, bases, off)
    assert st["n_lanes"] == 3 and got == want
    assert_same_hits(dev_hits, hits)
    # (b) run_host, both modes, and a second run replaces the first's assignments
    b = M.Batch(ix, 0, n, len(bases))
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.run_host(bases, off)
    assert got_assignments(b) == want
    assert_same_hits(b.download(), hits)
    b.set_assignments(M.ASSIGN_ONLY)
    b.run_host(bases, off)
    assert got_assignments(b) == want
    assert len(b.download()) == 0 and b.stats()["n_hits"] == len(hits)
    # a host batch in ASSIGN_ONLY kept none of its hits: leaving the mode without a new run does not hand out stale ones
    b.set_assignments(M.ASSIGN_WITH_HITS)
    with pytest.raises(M.MtsvError) as e:
        b.download()
    assert e.value.code == _lib.E_ARG
    assert got_assignments(b) == want
    b.set_assignments(M.ASSIGN_ONLY)
    h = 1000
    b.run_host(bases[: int(off[h])], off[: h + 1])
    assert got_assignments(b) == [t for t in want if t[0] < h]
    # (c) run_host_parts in uneven pieces, an empty one among them
    cuts = [0, 7, 7, 40_001, 40_002, 77_777, n]
    parts = [(bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a]) for a, c in zip(cuts, cuts[1:])]
    b.run_host_parts(parts)
    assert got_assignments(b) == want
    assert got_assignments(b) == want                       # a download does not consume them
    b.close()
    # (d) a workspace so small that the batch takes many passes
    b = M.Batch(ix, 0, 3000, 3000 * 150)
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.run_host(bases, off)
    assert b.stats()["n_passes"] >= 30
    assert got_assignments(b) == want
    assert_same_hits(b.download(), hits)
    b.close()


def test_passes_that_are_run_again_contribute_once(tricky):
    ix, orc, reads = tricky[:3]
    reads = [r for r in reads if len(r) <= 253]
    mp, op = both_params(seed_size=11, seed_interval=4, max_hits=100000, tune_max_hits=100000, min_seed=0.1)
    bases, off = helpers.reads_to_batch(reads)
    want = A.collapse(oracle_hits(orc, bases, off, op))
    got, _, st = resident(ix, bases, off, mp, max_hits_ws=64)
    assert st["n_passes"] > 100
    assert got == want
    # the same reads twice on one workspace: the second run's assignments are not appended to the first's
    b = M.Batch(ix, 0, len(reads), len(bases), max_hits_ws=40000)
    b.set_assignments(M.ASSIGN_ONLY)
    b.upload(bases, off)
    b.run(mp)
    assert got_assignments(b) == want
    b.run(mp)
    assert got_assignments(b) == want
    b.close()


# ---- 4. tiers and edges ----

def test_tiers_at_their_edges(tiers, tricky, monkeypatch, capfd):
    ix, bases, off, hits, want, n = tiers
    per_read = collections.Counter(hits["read"].tolist())
    distinct = collections.Counter(r for r, _, _ in want)
    h = max(per_read.values())
    diff, later, same = K.duplicate_census(hits)
    assert h > 64 and len(want) < len(hits) and diff and later and same
    assert all(distinct[r] < c for r, c in per_read.items() if c > 64)
    assert sum(c == 1 for c in per_read.values()) > 50
    monkeypatch.setenv("MTSV_TRACE", "1")

    def run(env, ix=ix, bases=bases, off=off, hits=hits, want=want, n=n):
        for k in ("MTSV_COLLAPSE_LANE_MAX", "MTSV_COLLAPSE_WAVE_MAX", "MTSV_COLLAPSE_LDS_MAX"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv("MTSV_COLLAPSE_" + k, str(v))
        capfd.readouterr()
        got, _, _ = resident(ix, bases, off, mode=M.ASSIGN_ONLY)
        counts, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err)
        assert got == want, env
        assert (n_hits, n_assign) == (len(hits), len(want))
        lane_max, wave_max, lds_max = min(int(env.get("LANE_MAX", 16)), 16), min(int(env.get("WAVE_MAX", 64)), 64), int(env.get("LDS_MAX", 4096))
        lds_max = 1 << (lds_max.bit_length() - 1)                # a power of two: anything else is rounded down to one
        assert edges == (lane_max, wave_max, lds_max), env
        assert counts == expected_tiers(hits, n, lane_max, wave_max, lds_max), env
        return counts

    n_big = sum(c > 64 for c in per_read.values())
    assert n_big >= 100
    c = run({})
    assert c[0] > 50 and c[2] == n_big and c[3] == 0            # the LDS tier takes the heavy reads
    c = run({"LDS_MAX": 64})
    assert c[2] == 0 and c[3] == n_big                           # ... now the global tier does
    # (the three edges the wavefront tier is asked at all clip to 64 for reads of about 120 hits and are one case here: they
    #  stay as the cases set for this database; test_wavefront_tier_with_more_than_32_keys moves the edge across a count reads have)
    for w in (h - 1, h, h + 1):
        c = run({"LDS_MAX": 128, "WAVE_MAX": min(w, 64)})
        assert c[2] == n_big and c[3] == 0
    for lm in (1, 4):
        c = run({"LANE_MAX": lm})
        assert c[0] > 50 and c[2] == n_big
    # a power of two is taken as it is, anything else rounded down to one
    c = run({"LDS_MAX": 100, "WAVE_MAX": 8, "LANE_MAX": 2})
    assert c[2] == 0 and c[3] == n_big
    # the tricky database: the lane tier's edge at a hit count its reads have, and the wavefront tier behind it
    tix, torc, treads = tricky[:3]
    tb, to = helpers.reads_to_batch(treads)
    th = oracle_hits(torc, tb, to)
    tw = A.collapse(th)
    tcount = collections.Counter(collections.Counter(th["read"].tolist()).values())
    cc = max((k for k in tcount if 2 < k <= 16), key=lambda k: tcount[k])
    for lm in (cc - 1, cc, cc + 1):
        c = run({"LANE_MAX": lm}, tix, tb, to, th, tw, len(treads))
        assert (c[1] >= tcount[cc]) == (lm == cc - 1)
        assert c[0] > 0
    assert tcount[2] and cc <= 8 and max(tcount) <= 16
    c = run({"LANE_MAX": 1, "WAVE_MAX": cc - 1, "LDS_MAX": 16}, tix, tb, to, th, tw, len(treads))
    assert c[0] and c[1] and c[2] >= tcount[cc] and not c[3]     # lane, wavefront and LDS tiers in one run
    c = run({"LANE_MAX": 1, "WAVE_MAX": 2, "LDS_MAX": 2}, tix, tb, to, th, tw, len(treads))
    assert c[0] and c[1] and not c[2] and c[3] >= tcount[cc]     # ... and the global tier behind the wavefront tier


def test_wavefront_tier_with_more_than_32_keys(tmp_path, monkeypatch, capfd):
    """reads of 60 hits on 45 TaxIDs: the wavefront tier with keys in the upper lanes, and its edge at that count"""
    entries, seg, rng = K.wave_db()
    ix, orc = built(entries, tmp_path, "wave")
    reads = K.tier_reads(rng, seg, 60) + K.background_reads(rng, entries[:3], 70)
    random.Random(8).shuffle(reads)
    bases, off = helpers.reads_to_batch(reads)
    hits = oracle_hits(orc, bases, off)
    want = A.collapse(hits)
    per_read = collections.Counter(hits["read"].tolist())
    h = max(per_read.values())
    n_big = sum(c == h for c in per_read.values())
    diff, later, same = K.duplicate_census(hits)
    assert 32 < h < 64 and n_big >= 50 and len(want) < len(hits) and diff and later and same
    monkeypatch.setenv("MTSV_TRACE", "1")
    for env, tier in (({}, 1), ({"WAVE_MAX": h - 1}, 2), ({"WAVE_MAX": h}, 1), ({"WAVE_MAX": h + 1}, 1),
                      ({"WAVE_MAX": h - 1, "LDS_MAX": 32}, 3), ({"LANE_MAX": 1, "WAVE_MAX": 64}, 1)):
        for k in ("LANE_MAX", "WAVE_MAX", "LDS_MAX"):
            monkeypatch.delenv("MTSV_COLLAPSE_" + k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv("MTSV_COLLAPSE_" + k, str(v))
        capfd.readouterr()
        got, _, _ = resident(ix, bases, off, mode=M.ASSIGN_ONLY)
        counts, edges, n_hits, n_assign = traced_tiers(capfd.readouterr().err)
        assert got == want, env
        assert counts == expected_tiers(hits, len(reads), *edges), env
        assert counts[tier] == n_big, env


# ---- 5. off is off, and refusals ----

def test_off_is_off_and_refusals(tricky):
    ix, orc, reads = tricky[:3]
    bases, off = helpers.reads_to_batch(reads)
    hits = oracle_hits(orc, bases, off)
    want = A.collapse(hits)
    n = len(reads)
    plain = M.Batch(ix, 0, n, len(bases))
    plain.upload(bases, off)
    plain.run()
    with pytest.raises(M.MtsvError) as e:
        plain.download_assignments()
    assert e.value.code == _lib.E_ARG
    on = M.Batch(ix, 0, n, len(bases))
    on.set_assignments(M.ASSIGN_WITH_HITS)
    on.upload(bases, off)
    on.run()
    assert_same_hits(plain.download(), hits)
    assert_same_hits(on.download(), hits)
    sp, so = plain.stats(), on.stats()
    assert {k: v for k, v in sp.items() if k.startswith("n_")} == {k: v for k, v in so.items() if k.startswith("n_")}
    # a bad mode; MATCH_ONLY then assignments, and the other way round
    for bad in (-1, 3):
        with pytest.raises(M.MtsvError) as e:
            plain.set_assignments(bad)
        assert e.value.code == _lib.E_ARG
    plain.set_match_flags(M.MATCH_ONLY)
    with pytest.raises(M.MtsvError) as e:
        plain.set_assignments(M.ASSIGN_ONLY)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(M.MtsvError) as e:
        on.set_match_flags(M.MATCH_ONLY)
    assert e.value.code == _lib.E_ARG
    assert got_assignments(on) == want                       # the refusal changed nothing
    # switched off again: the download is refused, and a run costs nothing of it
    on.set_assignments(M.ASSIGN_OFF)
    with pytest.raises(M.MtsvError) as e:
        on.download_assignments()
    assert e.value.code == _lib.E_ARG
    # the report and the flags beside ASSIGN_ONLY
    on.set_assignments(M.ASSIGN_ONLY)
    on.set_taxa_report(True)
    on.set_match_flags(M.MATCH_WITH_HITS)
    on.run()
    assert got_assignments(on) == want
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


# ---- 6. chain ----

def test_assignments_behind_a_filter_carry_the_callers_read_numbers(tricky, tmp_path):
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
    parts = [reads[i] for i in survivors]
    sb, so = helpers.reads_to_batch(parts)
    want_hits = oracle_hits(orc_d, sb, so)
    want_hits["read"] = survivors[want_hits["read"].astype(np.int64)]
    want = A.collapse(want_hits)
    assert len(want) > 20 and any(r != i for i, r in enumerate(sorted({t[0] for t in want})))
    src = M.Batch(ix_f, 0, n, len(bases))
    src.set_match_flags(M.MATCH_ONLY)
    src.upload(bases, off)
    src.run()
    for mode in (M.ASSIGN_WITH_HITS, M.ASSIGN_ONLY):
        dst = M.Batch(ix_d, 0, n, len(bases))
        dst.set_assignments(mode)
        taken = dst.take_reads(src, M.KEEP_UNMATCHED)
        assert taken[0] == len(survivors)
        dst.run()
        assert got_assignments(dst) == want
        if mode == M.ASSIGN_WITH_HITS:
            assert_same_hits(dst.download(), want_hits)
        dst.close()
    src.close()


# ---- 7. chunks ----

def test_collector_assignments_equal_mtsv_collapse_on_the_chunk_files(tmp_path):
    first, second, seg, rng = K.tier_db(split=True)
    (ix1, orc1), (ix2, orc2) = built(first, tmp_path, "c1"), built(second, tmp_path, "c2")
    reads = K.tier_reads(rng, seg, 60) + K.background_reads(rng, first[:2] + second[:1], 100)
    random.Random(6).shuffle(reads)
    bases, off = helpers.reads_to_batch(reads)
    n = len(reads)
    parts = [oracle_hits(o, bases, off) for o in (orc1, orc2)]
    assert {int(t) for t in parts[0]["tax_id"]} & {int(t) for t in parts[1]["tax_id"]}
    want = A.collapse(np.concatenate(parts))
    assert len(want) < len(parts[0]) + len(parts[1])
    ids = [f"read{i}" for i in range(n)]
    files = []
    for k, p in enumerate(parts):
        f = tmp_path / f"chunk{k}.results"
        f.write_text(M.format_results(p, ids))
        files.append(str(f))
    out = tmp_path / "collapsed.txt"
    r = subprocess.run([COLLAPSE, "-o", str(out), *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    srcs = [M.Batch(ix, 0, n, len(bases)) for ix in (ix1, ix2)]
    srcs[0].upload(bases, off)
    srcs[1].copy_reads(srcs[0])
    for s in srcs:
        s.run()
    dst = M.Batch(ix1, 0, 64, 1 << 12)
    dst.set_assignments(M.ASSIGN_WITH_HITS)
    dst.merge_runs(srcs)
    assert got_assignments(dst) == want
    a, _ = dst.download_assignments()
    assert sorted(M.format_assignments(a, ids).splitlines()) == sorted(out.read_text().splitlines())
    assert len(dst.download()) == len(parts[0]) + len(parts[1])
    # a refused merge leaves the collector's assignments readable
    srcs[1].set_match_flags(M.MATCH_ONLY)
    with pytest.raises(M.MtsvError) as e:
        dst.merge_runs(srcs)
    assert e.value.code == _lib.E_ARG
    assert got_assignments(dst) == want
    # ASSIGN_ONLY on the collector; a merge of one source is that run
    srcs[1].set_match_flags(M.MATCH_OFF)
    dst.set_assignments(M.ASSIGN_ONLY)
    dst.merge_runs(srcs[:1])
    assert got_assignments(dst) == A.collapse(parts[0])
    assert len(dst.download()) == 0 and dst.stats()["n_hits"] == len(parts[0])
    for b in srcs + [dst]:
        b.close()


# ---- 8. command line ----

BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """the golden reads as FASTQ; the golden database whole, cut into two chunk indexes, and a filter of unrelated
    sequences (it removes no read: the lines stay the golden ones)"""
    d = tmp_path_factory.mktemp("assign_cli")
    reads = [l.rstrip("\n") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    fq = d / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i} desc\n{r}\n+\n{'I' * len(r)}\n")
    db_fasta = os.path.join(GOLD, "e2e_db.fasta")
    lines = open(db_fasta).read().splitlines(keepends=True)
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
    # a database binned in two chunks is not the database binned whole (the cut-offs of the selection loop are per index):
    # what --merge-on-gpu must write comes from the oracle on the two chunks, collapsed over both
    bases, off = helpers.reads_to_batch([r.encode("latin-1") for r in reads])
    parts = np.concatenate([oracle_hits(O.Index.read(paths[c]), bases, off) for c in ("a", "b")])
    chunk_lines = sorted(A.text(A.collapse(parts), [f"r{i}" for i in range(len(reads))]).splitlines())
    return fq, paths, chunk_lines


CLI_VARIANTS = {
    "plain": lambda p: (["-i", p["D"]], False),
    "two_workers": lambda p: (["-i", p["D"], "--devices", "0,0"], False),
    "batch_reads_9": lambda p: (["-i", p["D"], "--batch-reads", "9"], False),
    "report": lambda p: (["-i", p["D"]], True),
    "filter_index": lambda p: (["-i", p["D"], "--filter-index", p["F"]], False),
    "merge_on_gpu": lambda p: (["-i", p["a"] + "," + p["b"], "--merge-on-gpu"], True),
}


@pytest.mark.parametrize("variant", list(CLI_VARIANTS))
def test_cli_writes_the_same_file_from_assignments(cli, variant, tmp_path):
    fq, paths, chunk_lines = cli
    args, with_report = CLI_VARIANTS[variant](paths)
    want = sorted(open(os.path.join(GOLD, "e2e_default.results")).read().splitlines())
    if variant == "merge_on_gpu":
        assert chunk_lines != want and len(chunk_lines) == len(want)
        want = chunk_lines
    out = {}
    for setting in ("1", "0"):
        res, rep = tmp_path / f"res{setting}.txt", tmp_path / f"rep{setting}.tsv"
        extra = ["--report", rep] if with_report else []
        r = run_binner("--fastq", fq, *args, "-m", res, *extra, env={"MTSV_CLI_ASSIGN": setting, "MTSV_TRACE": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("[collapse]" in r.stderr) == (setting == "1")      # the setting is what decides which path wrote the file
        out[setting] = (res.read_bytes(), rep.read_bytes() if with_report else b"")
    assert out["1"] == out["0"]                                 # byte for byte: the lines are written in input order
    assert sorted(out["1"][0].decode().splitlines()) == sorted(out["0"][0].decode().splitlines()) == want
    assert out["1"][1] == out["0"][1]


def test_cli_long_format_stays_on_hits(cli, tmp_path):
    fq, paths, _ = cli
    res = tmp_path / "long.txt"
    r = run_binner("--fastq", fq, "-i", paths["D"], "-m", res, "--output-format", "long", env={"MTSV_CLI_ASSIGN": "1", "MTSV_TRACE": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[collapse]" not in r.stderr
    assert sorted(res.read_text().splitlines()) == sorted(open(os.path.join(GOLD, "e2e_default_long.results")).read().splitlines())
