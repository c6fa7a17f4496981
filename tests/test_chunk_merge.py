"""-m gpu tests of chunked databases on one GPU (k_merge.hip, mtsv_batch_copy_reads / mtsv_batch_merge_runs, mtsv-binner
--merge-on-gpu): the same reads in a workspace per chunk, the chunks' hits merged per read in HBM, report and flags of the
merge.

Expected values always come from the CPU oracle: O.Index.build(chunk).bin_batch per chunk, put together per read in chunk
order by the restatement (chunk_merge_ref.py), then taxa_report_ref.classify_hits -- never from the device's own hits.
Every comparison is exact."""
import os
import random
import subprocess

import numpy as np
import pytest

import chunk_merge_ref as CM
import helpers
import mtsv_tools_amd as M
import taxa_report_ref as R
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_partition_cpu import write_input
from test_read_chain import sub_batch_arrays
from test_taxa_report import PARAM_SETS, both_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
COLLAPSE = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
PARTITION = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-partition")
MERGE_PARAMS = ("default", "stress", "one_assignment", "loose")
N_SYNTH = 100_003          # many scan tiles, several workgroups, a last flag word that is not full
N_PLANTED = 300


class Chunked:
    """a database cut into chunks, the same reads for all of them, and the oracle's word on every chunk (cached per
    parameter set: computed once, shared by the tests, never changed)"""

    def __init__(self, name, orcs, bases, off, entries=None):
        self.name, self.orcs, self.bases, self.off, self.entries = name, orcs, bases, off, entries
        self.n = len(off) - 1
        self.k = len(orcs)
        self.ixs = None
        self._want = {}

    def parts(self, pname="default"):
        if pname not in self._want:
            _, op = both_params(**PARAM_SETS[pname])
            ps = [orc.bin_batch(self.bases, self.off, op, threads=16)[0] for orc in self.orcs]
            self._want[pname] = (ps, CM.merge_hits(ps) if self.n < 10000 else merge_large(ps))
        return self._want[pname][0]

    def merged(self, pname="default"):
        self.parts(pname)
        return self._want[pname][1]


def merge_large(parts):
    """the restatement's result for lists too long for its loops: chunk order kept inside a read by a stable sort"""
    cat = np.concatenate(parts)
    return cat[np.argsort(cat["read"], kind="stable")]


def make_tricky3():
    entries, gene, unit = helpers.tricky_db(seed=7)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=40, lengths=(150, 320))
    bases, off = helpers.reads_to_batch(reads)
    chunks = [entries[c::3] for c in range(3)]
    fx = Chunked("tricky3", [O.Index.build(ch) for ch in chunks], bases, off, chunks)
    fx.reads = reads
    return fx


def check_tricky3(fx):
    parts, merged = fx.parts(), fx.merged()
    assert fx.n == 237
    per_chunk = sum(R.classify_hits(p)[1] for p in parts)
    assert (R.classify_hits(merged)[1], per_chunk) == (182, 341)             # per-chunk counters do not add up
    several, differ, only, none = CM.chunk_facts(parts, fx.n)
    assert (several, differ, only, none) == (80, 78, [62, 16, 24], 55)
    taxa0 = {e[0] for e in fx.entries[0]}
    union = {e[0] for ch in fx.entries for e in ch}
    fx.absent_from_0 = sorted(union - taxa0)
    assert fx.absent_from_0


def make_planted5(n_reads=N_PLANTED):
    rng = random.Random(29)
    seg = helpers.rnd_seq(rng, 400)
    plants = []
    for k in range(192):
        copy = helpers.substitute(rng, seg, 2 * ((k // 96 + k) % 4))
        if k < 96 and k % 4 == 0:
            copy = helpers.revcomp(copy)
        plants.append((copy, [(1000 + k % 96, 5000 + k)]))
    background = [(7, 1, 3000), (8, 2, 3000), (9, 3, 3000)]
    entries = helpers.planted_db(rng, background, plants)
    reads = []
    for i in range(n_reads):
        if i % 3 == 2:
            s = entries[i % 3][2]
            st = rng.randrange(0, len(s) - 150)
            reads.append(s[st:st + 150])
        else:
            st = rng.randrange(0, len(seg) - 150)
            r = helpers.mutate(rng, seg[st:st + 150], rng.randrange(0, 5), b"ACGT")
            reads.append(r if i % 2 else helpers.revcomp(r))
    bases, off = helpers.reads_to_batch(reads)
    chunks = [entries[c::5] for c in range(5)]
    return Chunked("planted5", [O.Index.build(ch) for ch in chunks], bases, off, chunks)


def check_planted5(fx):
    parts, merged = fx.parts(), fx.merged()
    per_read = np.bincount(merged["read"].astype(np.int64), minlength=fx.n)
    seg_reads = np.array([i % 3 != 2 for i in range(fx.n)])
    n_seg = int(seg_reads.sum())
    # reads of the segment: a hit in every one of the 192 plants, but for one read that an edit near its end costs one of
    # the plants with six substitutions (the oracle's figures for these 300 reads)
    assert fx.n == 300 and n_seg == 200
    assert int((per_read[seg_reads] == 192).sum()) == 199 and int((per_read[seg_reads] == 191).sum()) == 1
    several, differ, only, none = CM.chunk_facts(parts, fx.n)
    assert differ == n_seg and several == n_seg
    assert int((per_read == 1).sum()) == fx.n - n_seg                        # the background reads: one hit


def to_device(fx):
    fx.ixs = []
    for ch in fx.entries:
        ix = M.MGIndex.build(ch, threads=4)
        ix.to_device(0)
        fx.ixs.append(ix)
    return fx


@pytest.fixture(scope="module")
def tricky3():
    fx = make_tricky3()
    check_tricky3(fx)
    return to_device(fx)


@pytest.fixture(scope="module")
def planted5():
    fx = make_planted5()
    check_planted5(fx)
    return to_device(fx)


@pytest.fixture(scope="module")
def synth2(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth2")
    ixs, orcs, halves = [], [], []
    for c, seed in enumerate((5, 6)):
        ix = M.MGIndex.synth(seed=seed, n_taxa=12, gis_per_taxon=2, seq_len=20000)
        p = str(d / f"s{c}.idx")
        ix.write(p)
        ix.to_device(0)
        ixs.append(ix)
        orcs.append(O.Index.read(p))
        b, o = M.synth_reads(ix, seed=9 + c, n_reads=N_SYNTH // 2 + 1 - c, read_len=150)
        assert np.array_equal(np.diff(o.astype(np.int64)), np.full(len(o) - 1, 150))
        halves.append(np.asarray(b).reshape(-1, 150))
    rows = np.empty((N_SYNTH, 150), dtype=np.uint8)                          # drawn from both chunks in turn
    rows[0::2] = halves[0]
    rows[1::2] = halves[1]
    bases = rows.reshape(-1)
    off = np.arange(N_SYNTH + 1, dtype=np.uint64) * 150
    fx = Chunked("synth2", orcs, bases, off)
    fx.ixs = ixs
    pres = [CM.presence(p, fx.n) for p in fx.parts()]
    assert pres[0].any() and pres[1].any() and not (pres[0] | pres[1]).all() and N_SYNTH % 64 != 0
    return fx


def run_sources(fx, mp=None, vmode=0, n=None, bases=None, off=None, **kw):
    """upload to chunk 0's workspace, copy_reads to the others, a run on each"""
    bases = fx.bases if bases is None else bases
    off = fx.off if off is None else off
    n = len(off) - 1
    srcs = []
    for ix in fx.ixs:
        b = M.Batch(ix, 0, max(n, 1), max(len(bases), 1), **kw)
        b.set_verify_mode(vmode)
        srcs.append(b)
    srcs[0].upload(bases, off)
    for b in srcs[1:]:
        assert b.copy_reads(srcs[0]) >= 0.0
    for b in srcs:
        b.run(mp)
    return srcs


def collector(fx, flags=False, report=False):
    dst = M.Batch(fx.ixs[0], 0, 64, 1 << 12)
    if flags:
        dst.set_match_flags(M.MATCH_WITH_HITS)
    if report:
        dst.set_taxa_report(True)
    return dst


def close_all(*bs):
    for b in bs:
        b.close()


def report_of(b, reset=False):
    rows, total, ms = b.taxa_report(reset=reset)
    assert list(rows["tax_id"]) == sorted(set(rows["tax_id"].tolist())) and ms >= 0
    return R.rows_dict(rows), total


# ---- 1. merged hits ----

@pytest.mark.parametrize("vmode", [0, 1], ids=["reference", "edit_first"])
@pytest.mark.parametrize("pname", MERGE_PARAMS)
@pytest.mark.parametrize("which", ["tricky3", "planted5"])
def test_merged_hits_equal_the_oracle(which, pname, vmode, request):
    fx = request.getfixturevalue(which)
    mp, _ = both_params(**PARAM_SETS[pname])
    srcs = run_sources(fx, mp, vmode)
    dst = collector(fx)
    assert dst.merge_runs(srcs) >= 0.0
    want = fx.merged(pname)
    assert len(want) > 0
    assert_same_hits(dst.download(), want)
    st = dst.stats()
    assert (st["n_reads"], st["n_hits"]) == (fx.n, len(want))
    assert all(v == 0 for k, v in st.items() if k not in ("n_reads", "n_hits", "stage_ms")) and not any(st["stage_ms"].values())
    for b, p in zip(srcs, fx.parts(pname)):                                  # the sources keep their own results
        assert_same_hits(b.download(), p)
    assert_same_hits(dst.download(), want)                                   # ... and the merge can be downloaded again
    close_all(dst, *srcs)


def test_merged_hits_of_100003_reads_equal_the_oracle(synth2):
    fx = synth2
    srcs = run_sources(fx)
    dst = collector(fx, flags=True)
    dst.merge_runs(srcs)
    want = fx.merged()
    assert_same_hits(dst.download(), want)
    flags, n_matched = dst.match_flags()
    pres = CM.presence(want, fx.n)
    assert np.array_equal(flags, pres) and n_matched == int(pres.sum())
    for b, p in zip(srcs, fx.parts()):
        assert_same_hits(b.download(), p)
    close_all(dst, *srcs)


# ---- 2. sources of several passes ----

def test_sources_of_several_passes_give_the_same_merge(tricky3):
    fx = tricky3
    srcs = run_sources(fx, max_hits_ws=64)
    assert all(b.stats()["n_passes"] > 1 for b in srcs)
    dst = collector(fx, flags=True)
    dst.merge_runs(srcs)
    assert_same_hits(dst.download(), fx.merged())
    flags, n_matched = dst.match_flags()
    assert np.array_equal(flags, CM.presence(fx.merged(), fx.n)) and n_matched == 182
    close_all(dst, *srcs)


# ---- 3. the report of the merge ----

@pytest.mark.parametrize("dense_max", [None, "1"], ids=["dense", "hashed"])
@pytest.mark.parametrize("which", ["tricky3", "planted5"])
def test_report_of_the_merge_equals_the_classification_of_the_merged_hits(which, dense_max, request, monkeypatch):
    fx = request.getfixturevalue(which)
    if dense_max:
        monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", dense_max)
    stats, total = R.classify_hits(fx.merged())
    srcs = run_sources(fx)
    dst = collector(fx, report=True)                                         # on before the first merge
    dst.merge_runs(srcs)
    assert report_of(dst) == (stats, total)
    if which == "tricky3":
        assert total == 182
        absent = [t for t in fx.absent_from_0 if t in stats]
        assert absent and all(t in report_of(dst)[0] for t in absent)        # TaxIDs dst's own index does not hold
    # two merges add up, reset clears
    dst.merge_runs(srcs)
    twice = {t: [2 * v for v in row] for t, row in stats.items()}
    assert report_of(dst, reset=True) == (twice, 2 * total)
    assert report_of(dst) == ({}, 0)
    dst.merge_runs(srcs)
    assert report_of(dst) == (stats, total)
    close_all(dst, *srcs)


def test_report_switched_on_between_two_merges_counts_the_second(tricky3):
    fx = tricky3
    stats, total = R.classify_hits(fx.merged())
    srcs = run_sources(fx)
    dst = collector(fx)
    dst.merge_runs(srcs)
    with pytest.raises(M.MtsvError):
        dst.taxa_report()
    dst.set_taxa_report(True)
    assert report_of(dst) == ({}, 0)
    dst.merge_runs(srcs[:1])                                                 # chunk 0 alone first: the list is dst's own index's
    s0, t0 = R.classify_hits(fx.parts()[0])
    assert report_of(dst) == (s0, t0)
    dst.merge_runs(srcs)                                                     # now the other chunks bring their TaxIDs: rebuilt, counts kept
    both = {t: list(row) for t, row in stats.items()}
    for t, row in s0.items():
        both[t] = [a + b for a, b in zip(both.get(t, [0, 0, 0, 0]), row)]
    assert report_of(dst) == (both, total + t0)
    close_all(dst, *srcs)


# ---- 4. the flags of the merge ----

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 237])
def test_flags_of_the_merge_on_prefixes(tricky3, n):
    fx = tricky3
    o = fx.off[:n + 1]
    b = fx.bases[:int(o[-1])]
    parts = [p[p["read"] < n] for p in fx.parts()]                            # (a read's hits do not depend on the reads beside it)
    want = CM.merge_hits(parts)
    srcs = run_sources(fx, bases=b, off=o)
    dst = collector(fx, flags=True)
    dst.merge_runs(srcs)
    assert_same_hits(dst.download(), want)
    flags, n_matched = dst.match_flags()
    pres = CM.presence(want, n)
    assert len(flags) == n and np.array_equal(flags, pres) and n_matched == int(pres.sum())
    close_all(dst, *srcs)


def test_flags_of_reads_without_any_hit_and_of_a_source_without_hits(tricky3):
    fx = tricky3
    pres = [CM.presence(p, fx.n) for p in fx.parts()]
    none = np.nonzero(~(pres[0] | pres[1] | pres[2]))[0]
    assert len(none) == 55
    b, o = sub_batch_arrays(fx.bases, fx.off, none)
    srcs = run_sources(fx, bases=b, off=o)
    dst = collector(fx, flags=True, report=True)
    dst.merge_runs(srcs)
    flags, n_matched = dst.match_flags()
    assert len(flags) == 55 and not flags.any() and n_matched == 0 and len(dst.download()) == 0
    assert dst.stats()["n_hits"] == 0 and report_of(dst) == ({}, 0)
    close_all(*srcs)
    # reads chunk 1 has nothing for, which chunks 0 and 2 match: one source without any hit among sources with hits
    idx = np.nonzero(~pres[1] & (pres[0] | pres[2]))[0]
    assert pres[0][idx].any() and pres[2][idx].any()
    b, o = sub_batch_arrays(fx.bases, fx.off, idx)
    pos = {int(r): k for k, r in enumerate(idx)}
    parts = []
    for p in fx.parts():
        q = p[np.isin(p["read"], idx)].copy()
        q["read"] = [pos[int(r)] for r in q["read"]]
        parts.append(q)
    assert len(parts[1]) == 0
    srcs = run_sources(fx, bases=b, off=o)
    assert len(srcs[1].download()) == 0
    dst.merge_runs(srcs)
    want = CM.merge_hits(parts)
    assert_same_hits(dst.download(), want)
    flags, n_matched = dst.match_flags()
    assert flags.all() and n_matched == len(idx)
    assert report_of(dst) == R.classify_hits(want)
    close_all(dst, *srcs)


# ---- 5. one source ----

def test_merge_of_one_source_is_that_run(tricky3):
    fx = tricky3
    srcs = run_sources(fx)
    dst = collector(fx, flags=True)
    dst.merge_runs(srcs[2:])
    want = fx.parts()[2]
    assert_same_hits(dst.download(), want)
    flags, n_matched = dst.match_flags()
    pres = CM.presence(want, fx.n)
    assert np.array_equal(flags, pres) and n_matched == int(pres.sum())
    close_all(dst, *srcs)


# ---- 6. copy_reads ----

def test_copy_reads_after_upload_and_after_take_reads(tricky3):
    fx = tricky3
    a = M.Batch(fx.ixs[0], 0, fx.n, len(fx.bases))
    a.set_match_flags(M.MATCH_WITH_HITS)
    a.upload(fx.bases, fx.off)
    b = M.Batch(fx.ixs[1], 0, fx.n, len(fx.bases))
    b.copy_reads(a)                                                          # no run, no flags needed
    ca, oa = a.download_reads()
    cb, ob = b.download_reads()
    assert np.array_equal(ca, cb) and np.array_equal(oa, ob) and np.array_equal(b.read_map(), np.arange(fx.n, dtype=np.uint64))
    b.run()
    assert_same_hits(b.download(), fx.parts()[1])
    # mapped: the reads chunk 0 does not match, taken into c, copied into d
    a.run()
    c = M.Batch(fx.ixs[1], 0, fx.n, len(fx.bases))
    d = M.Batch(fx.ixs[2], 0, fx.n, len(fx.bases))
    kept, _, _ = c.take_reads(a, M.KEEP_UNMATCHED)
    surv = np.nonzero(~CM.presence(fx.parts()[0], fx.n))[0]
    assert kept == len(surv) and 0 < kept < fx.n
    d.copy_reads(c)
    cc, oc = c.download_reads()
    cd, od = d.download_reads()
    assert np.array_equal(cc, cd) and np.array_equal(oc, od)
    assert np.array_equal(d.read_map(), c.read_map()) and np.array_equal(d.read_map(), surv.astype(np.uint64))
    d.run()
    p2 = fx.parts()[2]
    assert_same_hits(d.download(), p2[np.isin(p2["read"], surv)])             # the caller's read numbers
    # a copy from a copy; upload on a copy drops the map
    e = M.Batch(fx.ixs[0], 0, fx.n, len(fx.bases))
    e.copy_reads(d)
    assert np.array_equal(e.read_map(), surv.astype(np.uint64))
    e.upload(fx.bases, fx.off)
    assert np.array_equal(e.read_map(), np.arange(fx.n, dtype=np.uint64))
    e.run()
    assert_same_hits(e.download(), fx.parts()[0])
    # a host batch that fitted one segment is a source too
    h = M.Batch(fx.ixs[1], 0, fx.n, len(fx.bases))
    h.run_host(fx.bases, fx.off)
    e.copy_reads(h)
    ce, oe = e.download_reads()
    assert np.array_equal(ce, ca) and np.array_equal(oe, oa)
    e.run()
    assert_same_hits(e.download(), fx.parts()[0])
    close_all(a, b, c, d, e, h)


def test_chunks_behind_a_filter(tricky3):
    """a filter index (every fourth sequence of the database plus unrelated ones), its unmatched reads into chunk 0's
    workspace, copied to the others, runs, merge: the caller's read numbers, flags per resident read"""
    fx = tricky3
    rng = random.Random(2024)
    every = [e for ch in fx.entries for e in ch]
    f_entries = every[::4] + [(700000 + k, 90000 + k, helpers.rnd_seq(rng, 2500)) for k in range(3)]
    f_ix = M.MGIndex.build(f_entries, threads=4)
    f_ix.to_device(0)
    f_want, _ = O.Index.build(f_entries).bin_batch(fx.bases, fx.off, O.default_params(), threads=16)
    in_f = CM.presence(f_want, fx.n)
    surv = np.nonzero(~in_f)[0]
    assert 0 < len(surv) < fx.n
    sb, so = sub_batch_arrays(fx.bases, fx.off, surv)
    parts = []
    for orc in fx.orcs:
        w, _ = orc.bin_batch(sb, so, O.default_params(), threads=16)
        parts.append(w)
    local = CM.merge_hits(parts)
    want = local.copy()
    want["read"] = surv[local["read"].astype(np.int64)]
    assert len(want) > 0 and len(set(local["read"].tolist())) < len(surv)
    f = M.Batch(f_ix, 0, fx.n, len(fx.bases))
    f.set_match_flags(M.MATCH_ONLY)
    f.upload(fx.bases, fx.off)
    f.run()
    srcs = [M.Batch(ix, 0, fx.n, len(fx.bases)) for ix in fx.ixs]
    kept, _, _ = srcs[0].take_reads(f, M.KEEP_UNMATCHED)
    assert kept == len(surv)
    for b in srcs[1:]:
        b.copy_reads(srcs[0])
    for b in srcs:
        b.run()
    dst = collector(fx, flags=True, report=True)
    dst.merge_runs(srcs)
    assert_same_hits(dst.download(), want)
    flags, n_matched = dst.match_flags()
    pres = CM.presence(local, len(surv))
    assert np.array_equal(flags, pres) and n_matched == int(pres.sum())
    assert np.array_equal(srcs[1].read_map(), surv.astype(np.uint64))
    assert report_of(dst) == R.classify_hits(want)
    close_all(dst, f, *srcs)


# ---- 7. refusals ----

def test_refusals_leave_the_destination_as_it_was(tricky3):
    fx = tricky3
    srcs = run_sources(fx)
    dst = collector(fx, flags=True)
    dst.merge_runs(srcs[:2])
    before = CM.merge_hits(fx.parts()[:2])
    flags_before = CM.presence(before, fx.n)

    def refused(call):
        with pytest.raises(M.MtsvError) as e:
            call()
        assert e.value.code == _lib.E_ARG, e.value
        assert_same_hits(dst.download(), before)
        flags, _ = dst.match_flags()
        assert np.array_equal(flags, flags_before)

    nb = len(fx.bases)
    refused(lambda: dst.merge_runs([srcs[0], dst]))                           # dst among the sources
    fresh = M.Batch(fx.ixs[1], 0, fx.n, nb)
    fresh.upload(fx.bases, fx.off)
    refused(lambda: dst.merge_runs([srcs[0], fresh]))                         # no completed run
    host = M.Batch(fx.ixs[1], 0, fx.n, nb)
    host.run_host(fx.bases, fx.off)
    refused(lambda: dst.merge_runs([srcs[0], host]))                          # last input a host batch
    only = M.Batch(fx.ixs[1], 0, fx.n, nb)
    only.set_match_flags(M.MATCH_ONLY)
    only.upload(fx.bases, fx.off)
    only.run()
    refused(lambda: dst.merge_runs([srcs[0], only]))                          # a source in MATCH_ONLY
    fewer = M.Batch(fx.ixs[1], 0, fx.n, nb)
    fewer.upload(fx.bases[:int(fx.off[100])], fx.off[:101])
    fewer.run()
    refused(lambda: dst.merge_runs([srcs[0], fewer]))                         # different n_reads
    lens = np.diff(fx.off.astype(np.int64))
    i = int(np.nonzero((lens[:-1] > 0) & (lens[1:] > 0))[0][0])
    off2 = fx.off.copy()
    off2[i + 1] -= 1                                                         # the same bases, one boundary moved
    other = M.Batch(fx.ixs[1], 0, fx.n, nb)
    other.upload(fx.bases, off2)
    other.run()
    refused(lambda: dst.merge_runs([srcs[0], other]))                         # equal n_reads, different offsets
    refused(lambda: dst.merge_runs([]))                                       # n_srcs = 0
    taker = M.Batch(fx.ixs[1], 0, fx.n, nb)
    refused(lambda: taker.take_reads(dst, M.KEEP_UNMATCHED))                  # take_reads from a merged dst
    # dst in MATCH_ONLY
    d2 = M.Batch(fx.ixs[0], 0, fx.n, nb)
    d2.set_match_flags(M.MATCH_ONLY)
    d2.upload(fx.bases, fx.off)
    d2.run()
    f2, m2 = d2.match_flags()
    with pytest.raises(M.MtsvError) as e:
        d2.merge_runs(srcs)
    assert e.value.code == _lib.E_ARG
    f3, m3 = d2.match_flags()
    pres0 = CM.presence(fx.parts()[0], fx.n)
    assert np.array_equal(f2, f3) and np.array_equal(f2, pres0) and m2 == m3 == int(pres0.sum())
    # copy_reads: into itself, from an empty workspace, into one that is too small -- the destination keeps its batch
    keep = M.Batch(fx.ixs[2], 0, 100, int(fx.off[100]))
    keep.upload(fx.bases[:int(fx.off[100])], fx.off[:101])
    codes, roff = keep.download_reads()
    empty = M.Batch(fx.ixs[1], 0, fx.n, nb)
    for call in (lambda: keep.copy_reads(keep), lambda: keep.copy_reads(empty), lambda: keep.copy_reads(srcs[0])):
        with pytest.raises(M.MtsvError) as e:
            call()
        assert e.value.code == _lib.E_ARG
        c2, o2 = keep.download_reads()
        assert np.array_equal(c2, codes) and np.array_equal(o2, roff)
    # after all of it the sources still merge
    dst.merge_runs(srcs)
    assert_same_hits(dst.download(), fx.merged())
    close_all(dst, fresh, host, only, fewer, other, taker, d2, keep, empty, *srcs)


# ---- 8. the command line ----

@pytest.fixture(scope="module")
def cli(tricky3, tmp_path_factory):
    fx = tricky3
    d = tmp_path_factory.mktemp("merge_cli")
    paths = []
    for c, ix in enumerate(fx.ixs):
        p = str(d / f"chunk{c}.idx")
        ix.write(p)
        paths.append(p)
    recs = [(b"r%d" % i, b"", bytes(r), b"I" * len(r)) for i, r in enumerate(fx.reads)]
    fq = d / "reads.fastq"
    write_input(fq, recs, [r[0] for r in recs], True, False)
    return fx, d, ",".join(paths), fq, recs


def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


CLI_CASES = {
    "default": ([], {}),
    "batch_reads_64": (["--batch-reads", "64"], {}),
    "two_workers": (["--batch-reads", "64"], {"MTSV_CLI_WORKERS": "2"}),
    "clean_exit": ([], {"MTSV_CLI_CLEAN_EXIT": "1"}),
}


@pytest.mark.parametrize("case", list(CLI_CASES))
def test_binner_merge_on_gpu(cli, case, tmp_path):
    fx, d, index, fq, recs = cli
    extra, env = CLI_CASES[case]
    plain, res = tmp_path / "plain.txt", tmp_path / "res.txt"
    rep, m, u = tmp_path / "rep.tsv", tmp_path / "m.fq", tmp_path / "u.fq"
    r = run_binner("--fastq", fq, "-i", index, "-m", plain, *extra, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_binner("--fastq", fq, "-i", index, "-m", res, "--merge-on-gpu", "--report", rep, "--matched", m, "--unmatched", u, *extra, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert res.read_bytes() == plain.read_bytes() and len(res.read_bytes()) > 0
    # the results file is what the oracle's merged hits format to
    ids = [rc[0].decode() for rc in recs]
    assert res.read_text() == M.format_results(fx.merged(), ids)
    # the report: mtsv-collapse --report on that file, and the oracle's classification
    out, crep = tmp_path / "collapsed.txt", tmp_path / "crep.tsv"
    assert subprocess.run([COLLAPSE, "-o", str(out), "--report", str(crep), str(res)], capture_output=True).returncode == 0
    assert rep.read_bytes() == crep.read_bytes()
    stats, total = R.classify_hits(fx.merged())
    assert R.parse_report(rep.read_text()) == stats and total == 182
    # the partition: mtsv-partition on that file
    m2, u2 = tmp_path / "m2.fq", tmp_path / "u2.fq"
    assert subprocess.run([PARTITION, "--results", str(res), "--fastq", str(fq), "--matched", str(m2), "--unmatched", str(u2)],
                          capture_output=True).returncode == 0
    assert m.read_bytes() == m2.read_bytes() and u.read_bytes() == u2.read_bytes()
    assert m.read_bytes().count(b"\n+\n") == 182 and u.read_bytes().count(b"\n+\n") == 55
    # --matched / --unmatched without a results file
    if case == "default":
        m3, u3 = tmp_path / "m3.fq", tmp_path / "u3.fq"
        r = run_binner("--fastq", fq, "-i", index, "--merge-on-gpu", "--matched", m3, "--unmatched", u3)
        assert r.returncode == 0, r.stdout + r.stderr
        assert m3.read_bytes() == m.read_bytes() and u3.read_bytes() == u.read_bytes()
