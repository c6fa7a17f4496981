"""-m gpu: k_coalesce_heavy walks the sorted hits of a strand of 65..2048 seed hits by runs (k_coalesce.hip: walk_by_runs),
a thread per run of hits that are `ok` and lie in one bin, and falls back to the wavefront walk when a run is longer than
a thread should walk.  Hits and counters must be the oracle's and those of MTSV_HEAVY_WALK=serial for strands on both
sides of every edge (65, 256 / 257 hits in one run, 2048 / 2049, more than 8192), for strands in one bin, in two with the
boundary inside a window's reach, in hundreds of bins, for hopeless strands and with max_candidates below the strand's
candidate count; MTSV_TRACE tells which walk the strands took."""
import random
import re

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STATS = {"n_seed_hits": "H", "n_candidates": "n_cand", "n_verified": "n_sw", "window_bytes": "W", "n_hits": "R"}
# K = 18, G = 1: a read of L bases with a unique origin has L - 17 seed hits on one strand, all in one run
PARAMS = dict(seed_size=18, seed_interval=1, max_hits=1_000_000, tune_max_hits=1_000_000)
RUN_MAX = 256  # k_coalesce.hip: kRunMax


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


def walks(text):
    """(strands walked by runs, strands that fell back to the wavefront walk), summed over the lanes that reported"""
    m = re.findall(r"k_coalesce_heavy: (\d+) strands walked by runs, (\d+) by the wavefront walk", text)
    assert m, text[-2000:]
    return sum(int(a) for a, _ in m), sum(int(b) for _, b in m)


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    """three long unique sequences; a 22-mer planted in 300 short sequences of as many TaxIds (every seed of it hits 300
    bins), a 40-mer in 12; two neighbours in the text whose junction a read spans"""
    rng = random.Random(4097)
    many = helpers.rnd_seq(rng, 22)
    some = helpers.rnd_seq(rng, 40)
    bg = [(601, 11, 12000), (602, 12, 12000), (603, 13, 9000)]
    plants = [(many, [(1000 + i, 5000 + i) for i in range(300)]), (some, [(2000 + i // 2, 6000 + i) for i in range(12)])]
    entries = helpers.planted_db(rng, bg, plants)
    entries.append((3001, 7001, helpers.rnd_seq(rng, 500)))   # neighbours in the text (ascending TaxId)
    entries.append((3002, 7002, helpers.rnd_seq(rng, 500)))
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "heavy.idx")
    ix.write(p)
    return ix, O.Index.read(p), entries, many, some


def unique_reads(entries, rng, lengths):
    out = []
    for k, L in enumerate(lengths):
        t = entries[k % 2][2]
        st = rng.randrange(0, len(t) - L)
        r = t[st:st + L]
        out.append(r if k % 2 == 0 else helpers.revcomp(r))
    return out


def run_batch(ix, reads, mp, monkeypatch, capfd, serial=False, **kw):
    bases, off = helpers.reads_to_batch(reads)
    monkeypatch.setenv("MTSV_TRACE", "1")
    if serial:
        monkeypatch.setenv("MTSV_HEAVY_WALK", "serial")
    b = M.Batch(ix, 0, len(reads), len(bases), max_hits_ws=1 << 21, lanes=1, **kw)
    capfd.readouterr()
    b.upload(bases, off)
    b.run(mp)
    got, st = b.download(), b.stats()
    b.close()
    w = walks(capfd.readouterr().err)
    monkeypatch.delenv("MTSV_HEAVY_WALK", raising=False)
    monkeypatch.delenv("MTSV_TRACE")
    return got, st, w


def check(got, st, want, ctr):
    assert_same_hits(got, want)
    for s, o in STATS.items():
        assert st[s] == ctr[o], s


def test_one_run_strands_on_both_sides_of_every_edge(db, monkeypatch, capfd):
    """strands whose hits all merge into one window: 65 and 256 hits are one thread's run, 257 and 2048 take the wavefront
    walk inside the small-LDS kernel, 2049 and 8193 belong to the other instantiation and the scratch path"""
    ix, orc, entries, _, _ = db
    ix.to_device(0)
    mp, op = both_params(**PARAMS)
    rng = random.Random(1)
    by_runs = [65, 66, 100, RUN_MAX - 1, RUN_MAX]
    fallback = [RUN_MAX + 1, 300, 1000, 2047, 2048]
    others = [64, 2049, 8192, 8193]
    for hits, want_walks in ((by_runs, (len(by_runs), 0)), (fallback, (0, len(fallback))),
                             (by_runs + fallback + others, (len(by_runs), len(fallback)))):
        reads = unique_reads(entries, rng, [h + 17 for h in hits])
        bases, off = helpers.reads_to_batch(reads)
        want, ctr = orc.bin_batch(bases, off, op, threads=8)
        assert ctr["H"] == sum(hits)
        got, st, w = run_batch(ix, reads, mp, monkeypatch, capfd)
        check(got, st, want, ctr)
        assert w == want_walks
        got, st, w = run_batch(ix, reads, mp, monkeypatch, capfd, serial=True)
        check(got, st, want, ctr)
        assert w == (0, 0)


def multi_bin_reads(entries, many, some):
    rng = random.Random(2)
    a, b = entries[-2][2], entries[-1][2]
    out = []
    # hundreds of bins: 5 seeds x 300 copies = 1500 hits, 300 runs of 5; with a unique flank the read's own origin besides
    out += [many, helpers.revcomp(many), helpers.rnd_seq(rng, 30) + many + helpers.rnd_seq(rng, 30)]
    owner = next(e[2] for e in entries if many in e[2] and len(e[2]) < 1000)
    at = owner.find(many)
    out += [owner[max(0, at - 60):at + 22 + 60], helpers.revcomp(owner[max(0, at - 40):at + 62])]
    # a dozen bins, 23 seeds each: 276 hits
    out += [some, helpers.revcomp(some), helpers.mutate(rng, some + many, 2, b"ACGT")]
    # two bins, the boundary inside a window's reach: a read over the junction of two neighbours in the text
    for k in (20, 50, 75, 100, 130):
        r = a[len(a) - k:] + b[:150 - k]
        out += [r, helpers.revcomp(r)]
    return out


def test_strands_in_two_and_in_hundreds_of_bins(db, monkeypatch, capfd):
    ix, orc, entries, many, some = db
    ix.to_device(0)
    reads = multi_bin_reads(entries, many, some)
    bases, off = helpers.reads_to_batch(reads)
    for extra in ({}, dict(min_seed=0.3), dict(max_candidates=2), dict(max_candidates=40, min_seed=0.02), dict(edit_rate=0.3)):
        mp, op = both_params(**PARAMS, **extra)
        want, ctr = orc.bin_batch(bases, off, op, threads=8)
        assert ctr["n_cand"] > 300 or extra.get("min_seed") == 0.3
        if "max_candidates" in extra:
            assert ctr["n_sw"] < ctr["n_cand"]      # max_candidates below the strands' candidate counts
        got, st, w = run_batch(ix, reads, mp, monkeypatch, capfd)
        check(got, st, want, ctr)
        assert w[0] >= len(reads) - 2 and w[1] == 0, w
        sgot, sst, sw = run_batch(ix, reads, mp, monkeypatch, capfd, serial=True)
        check(sgot, sst, want, ctr)
        assert sw == (0, 0)


def test_hopeless_heavy_strands(db, monkeypatch, capfd):
    """more N in the read than its edit tolerance: no candidate can pass, the strand's candidates are only accounted"""
    ix, orc, entries, many, some = db
    ix.to_device(0)
    rng = random.Random(3)
    reads = []
    for t in (entries[0][2], entries[1][2]):
        st = rng.randrange(0, len(t) - 253)
        r = t[st:st + 213] + b"N" * 40                       # ED = 33 < 40 N; 196 seed hits in one run
        reads += [r, helpers.revcomp(r)]
    reads += [many + b"N" * 30, b"N" * 30 + many + helpers.rnd_seq(rng, 20)]   # 1500 hits in 300 bins, ED = 7 / 10
    reads += [some + b"N" * 9 + many]                      # 276 + 1500 hits, ED = 10 > 9 N: not hopeless
    bases, off = helpers.reads_to_batch(reads)
    for extra in ({}, dict(max_candidates=3)):
        mp, op = both_params(**PARAMS, **extra)
        want, ctr = orc.bin_batch(bases, off, op, threads=8)
        assert ctr["n_cand"] > 600 and ctr["n_sw"] > 0
        got, st, w = run_batch(ix, reads, mp, monkeypatch, capfd)
        check(got, st, want, ctr)
        assert w[0] >= len(reads) and w[1] == 0, w
        sgot, sst, sw = run_batch(ix, reads, mp, monkeypatch, capfd, serial=True)
        check(sgot, sst, want, ctr)
        assert sw == (0, 0)


def test_host_path_with_three_lanes(db, monkeypatch, capfd):
    """run_host on a batch large enough for three lanes: every lane's passes walk their heavy strands by runs"""
    ix, orc, entries, many, some = db
    ix.to_device(0)
    rng = random.Random(5)
    unit = multi_bin_reads(entries, many, some) + unique_reads(entries, rng, [82, 150, RUN_MAX + 17, RUN_MAX + 18, 400])
    t = entries[2][2]
    while len(unit) < 400:                                     # ordinary reads in between
        st = rng.randrange(0, len(t) - 100)
        unit.append(t[st:st + rng.randrange(40, 100)])
    rng.shuffle(unit)
    reps = 3 * 32768 // len(unit) + 1
    mp, op = both_params(**PARAMS)
    ub, uo = helpers.reads_to_batch(unit)
    uwant, uctr = orc.bin_batch(ub, uo, op, threads=8)
    parts = []
    for k in range(reps):
        h = uwant.copy()
        h["read"] += k * len(unit)
        parts.append(h)
    want = np.concatenate(parts)
    ctr = {k: v * reps for k, v in uctr.items()}
    bases, off = helpers.reads_to_batch(unit * reps)
    assert len(off) - 1 >= 3 * 32768
    results = {}
    for serial in (False, True):
        monkeypatch.setenv("MTSV_TRACE", "1")
        if serial:
            monkeypatch.setenv("MTSV_HEAVY_WALK", "serial")
        b = M.Batch(ix, 0, len(off) - 1, len(bases), lanes=3)
        capfd.readouterr()
        b.run_host(bases, off, mp)
        got, st = b.download(), b.stats()
        b.close()
        w = walks(capfd.readouterr().err)
        monkeypatch.delenv("MTSV_HEAVY_WALK", raising=False)
        monkeypatch.delenv("MTSV_TRACE")
        assert st["n_lanes"] == 3
        check(got, st, want, ctr)
        results[serial] = w
    assert results[True] == (0, 0)
    assert results[False][0] > 10 * reps and results[False][1] >= 2 * reps
