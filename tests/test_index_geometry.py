"""-m gpu: the index geometry ladder (helpers.RUNGS) against the structures mtsv_index_to_device builds in HBM -- rank
blocks, the full suffix array, the k-mer table with its kept levels and tags, the coarse bin look-up -- and against the
prefix-doubling builder behind mtsv_set_build_device.  The rungs sit where that code branches on n (n % 128, the table
width, lut_shift, the packing threads), on the row of the sentinel, on the suffix sampling interval and on the
composition of the text.  Every rung is compared with the CPU oracle (test_index_geometry_cpu.py pins the oracle on the
same rungs first), hits and counters, and the position probes also with an expectation written in plain Python here that
knows nothing of FM indexes."""
import bisect
import random
from collections import Counter

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits, revcomp
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL_FLAGS = [M.DEV_SAMPLED_SA_ONLY | M.DEV_NO_KMER_TABLE, M.DEV_SAMPLED_SA_ONLY, M.DEV_NO_KMER_TABLE, M.DEV_DEFAULT]
DENSE = dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30)
# seeds short enough for the texts of the tiny rungs (those of test_tiny_index_of_the_reference_unit_test)
SMALL_SEEDS = (dict(seed_size=4, seed_interval=1, edit_rate=0.0), dict(seed_size=2, seed_interval=1, edit_rate=0.3),
               dict(seed_size=3, seed_interval=2, edit_rate=0.5, min_seed=1.0))
WIDTH_RUNGS = ("random-18", "random-128", "random-4096", "random-65537")


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


class Built:
    """one rung built once: its entries, text and bins, the product's host-built index, its file and the oracle's"""

    def __init__(self, rung, tmp):
        self.rung = rung
        self.entries = rung.entries()
        self.text = helpers.geometry_text(self.entries)
        self.starts, pos = [], 0
        for e in self.entries:
            self.starts.append(pos)
            pos += len(e[2])
        self.ix = M.MGIndex.build(self.entries, rung.occ_k, rung.sa_s, threads=4)
        self.path = str(tmp / (rung.name + ".idx"))
        self.ix.write(self.path)
        self.orc = O.Index.read(self.path)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("geometry")
    cache = {}

    def get(rung):
        if rung.name not in cache:
            cache[rung.name] = Built(rung, tmp)
        return cache[rung.name]

    yield get
    for b in cache.values():
        b.ix.close()


def upload(b, flags):
    """to_device, then the info every upload must report: n, the table width the rule of dev_index.hip gives for n, and
    whether the full suffix array is resident"""
    b.ix.to_device(0, flags)
    info = b.ix.info()
    assert info["n"] == b.rung.n and info["n_bins"] == len(b.entries), (flags, info)
    assert info["occ_k"] == b.rung.occ_k and info["sa_s"] == b.rung.sa_s, (flags, info)
    assert info["kmer_k"] == (0 if flags & M.DEV_NO_KMER_TABLE else helpers.kmer_width_for(b.rung.n)), (flags, info)
    assert info["sa_full"] == (0 if flags & M.DEV_SAMPLED_SA_ONLY else 1), (flags, info)


def run(ix, reads, mp, verify_mode=0, max_hits_ws=0):
    bases, off = helpers.reads_to_batch(reads)
    batch = M.Batch(ix, 0, len(reads), max(len(bases), 1), max_hits_ws)
    try:
        batch.set_verify_mode(verify_mode)
        batch.upload(bases, off)
        batch.run(mp)
        return batch.download(), batch.stats()
    finally:
        batch.close()


def assert_counters(st, ctr, sa_full, where):
    assert st["n_seed_hits"] == ctr["H"], where
    assert st["n_candidates"] == ctr["n_cand"], where
    assert st["n_verified"] == ctr["n_sw"], where
    assert st["window_bytes"] == ctr["W"], where
    assert st["n_hits"] == ctr["R"], where
    assert st["lf_steps"] == (0 if sa_full else ctr["S"]), where


def compare(b, reads, over, flags_list=ALL_FLAGS, verify_modes=(0,), max_hits_ws=0):
    """reads through the device index under every flag combination: hits and counters equal the oracle's; returns the
    oracle's hits and counters"""
    mp, op = both_params(**over)
    bases, off = helpers.reads_to_batch(reads)
    want, ctr = b.orc.bin_batch(bases, off, op, threads=8)
    for flags in flags_list:
        upload(b, flags)
        for vm in verify_modes:
            got, st = run(b.ix, reads, mp, vm, max_hits_ws)
            assert_same_hits(got, want)
            assert_counters(st, ctr, not flags & M.DEV_SAMPLED_SA_ONLY, (b.rung.name, flags, vm, over))
    return want, ctr


def tiny_extras(rng, text):
    """reads for texts too short to hold a probe, among them reads longer than the whole text"""
    out = [b"", b"A", b"ACGTACGTACGTACGTAC", b"N" * 24, text + b"ACGT", b"TT" + text, text * 2, text[:len(text) // 2],
           revcomp(text), text]
    return out + [helpers.rnd_seq(rng, 24) for _ in range(5)]


def python_expectation(b, probes):
    """{probe number: (tax_id, gi, edit, strand, offset)} of the probes whose answer plain Python knows: the probe lies
    wholly inside one sequence, holds no N, and its 24 symbols occur once in the text and not at all in the text's
    reverse complement.  At edit_rate 0 such a probe has exactly one hit: where it was cut."""
    text = b.text
    cnt = Counter(text[i:i + 24] for i in range(len(text) - 23))
    exp = {}
    for k, (i, read) in enumerate(probes):
        km = text[i:i + 24]
        if len(km) < 24 or 78 in km or cnt[km] != 1 or cnt.get(revcomp(km), 0) != 0:
            continue
        j = bisect.bisect_right(b.starts, i) - 1  # the last sequence that starts at or before i: empty ones lie before it
        tax, gi, seq = b.entries[j]
        if i + 24 > b.starts[j] + len(seq):
            continue
        exp[k] = (tax, gi, 0, k % 2, i - b.starts[j])
    return exp


def python_seed_hits(b, reads, mp):
    """n_seed_hits of reads that have one seed per strand (fewer symbols than seed_size + seed_interval): occurrences
    in the text of the first seed_size symbols of the read and of its reverse complement, counted by a plain scan"""
    K = mp.seed_size
    cnt = Counter(b.text[i:i + K] for i in range(len(b.text) - K + 1))
    total = 0
    for r in reads:
        assert len(r) < K + mp.seed_interval
        if len(r) >= K:
            for s in (r[:K], revcomp(r)[:K]):
                c = cnt.get(s, 0)
                total += c if c <= mp.max_hits else 0
    return total, cnt


@pytest.mark.parametrize("rung", helpers.RUNGS, ids=repr)
def test_position_probes(built, rung):
    """every 24-symbol substring of the text as a read at edit_rate 0: every row of the suffix array and every rank block
    answers for itself.  Oracle, counters, and on the random rungs the Python expectation."""
    b = built(rung)
    rng = random.Random(rung.n)
    probes = helpers.position_probes(b.text)
    reads = [r for _, r in probes]
    over = dict(edit_rate=0.0)
    if rung.n < 257:  # reads longer than the text, shorter than a seed, empty: the oracle and the counters only
        compare(b, tiny_extras(rng, b.text), over)
    if not reads:
        assert rung.n == 1
        return
    want, ctr = compare(b, reads, over)
    print(f"{rung.name}: {len(probes)} probes, {len(want)} hits, H={ctr['H']} S={ctr['S']}")
    h_py, cnt18 = python_seed_hits(b, reads, M.default_params(**over))
    assert ctr["H"] == h_py, (ctr["H"], h_py)
    if rung.kind != "random":
        return
    # the random rungs against plain Python.  The oracle's hits equal the device's (above), so they stand for both.
    with_seed = sum(1 for r in reads if len(r) >= 18)
    if all(c == 1 for c in cnt18.values()) and not any(revcomp(s) in cnt18 for s in cnt18):
        assert h_py == with_seed  # every 18-mer of the text is unique on both strands: one seed hit per probe with a seed
    else:
        assert h_py >= with_seed
    exp = python_expectation(b, probes)
    per_read = np.bincount(want["read"].astype(np.int64), minlength=len(reads))
    first = np.searchsorted(want["read"], np.arange(len(reads)))
    for k, e in exp.items():
        assert per_read[k] == 1, (k, probes[k], per_read[k])
        h = want[first[k]]
        assert (int(h["tax_id"]), int(h["gi"]), int(h["edit"]), int(h["strand"]), int(h["offset"])) == e, (k, probes[k], h, e)
    outside = len(probes) - len(exp)
    print(f"{rung.name}: {outside} of {len(probes)} probes outside the Python expectation")
    if rung.n >= 4095:
        assert outside <= 0.05 * len(probes), (outside, len(probes))


@pytest.mark.parametrize("rung", [r for r in helpers.RUNGS if r.n < 257], ids=repr)
def test_small_seeds_on_the_tiny_rungs(built, rung):
    """texts of fewer symbols than a default seed: every substring of up to 8 symbols, and reads longer than the text,
    with seeds of 2..4 symbols -- windows clipped at both ends of the only sequences, a text smaller than one rank
    block, a k-mer table as wide as the seed"""
    b = built(rung)
    rng = random.Random(rung.n + 1)
    reads = [r for _, r in helpers.position_probes(b.text, width=8)] + tiny_extras(rng, b.text)
    for over in SMALL_SEEDS:
        compare(b, reads, over, verify_modes=(0, 1))


@pytest.mark.parametrize("rung", [r for r in helpers.RUNGS if r.kind in ("sentinel", "nrun")], ids=repr)
def test_n_probes(built, rung, monkeypatch):
    """reads across every N run edge, their seeds holding 1..18 N: the only traffic that reads the derived rank of N
    (block_rank: rows before the block minus A+C+G+T minus the sentinel if it lies before the block)"""
    b = built(rung)
    if rung.kind == "sentinel":  # the rung is where it says: the product's own search agrees on the row (through the oracle's file)
        ok, lo, hi = b.orc.backward_search(b.text[:40])
        assert ok and hi - lo == 1 and lo == rung.sentinel_row()
    reads = helpers.n_edge_probes(random.Random(rung.n + 2), b.text)
    assert len(reads) >= 36 * 3 if rung.kind == "sentinel" else len(reads) == 36
    for edit_rate in (0.0, 0.13):
        want, ctr = compare(b, reads, dict(edit_rate=edit_rate), verify_modes=(0, 1))
        assert ctr["H"] > 0 and (len(want) > 0 or edit_rate == 0.0)  # (at edit_rate 0 a read's N is an edit too many)
    # and from the first symbol behind the last N instead of the kept table levels (a handle of its own: to_device
    # keeps what is resident when the flags are the same)
    mp, op = both_params(edit_rate=0.13)
    ix2 = M.MGIndex.load(b.path)
    monkeypatch.setenv("MTSV_KMER_LEVELS", "0")
    ix2.to_device(0, M.DEV_DEFAULT)
    monkeypatch.delenv("MTSV_KMER_LEVELS")
    got, st = run(ix2, reads, mp)
    ix2.close()
    assert_same_hits(got, want)
    assert_counters(st, ctr, True, (rung.name, "MTSV_KMER_LEVELS=0"))


@pytest.mark.parametrize("rung", [r for r in helpers.RUNGS if r.n >= 257], ids=repr)
def test_ordinary_reads(built, rung):
    """300 reads of 40..150 symbols with edits, default parameters, both verify orders; on the repeat rungs also the
    dense seeds with max_hits = 100000, which the default thinning would leave without a seed hit"""
    b = built(rung)
    reads = helpers.geometry_reads(random.Random(rung.n + 3), b.entries)
    assert len(reads) == 300 and min(map(len, reads)) >= 30 and max(map(len, reads)) <= 180
    want, ctr = compare(b, reads, {}, verify_modes=(0, 1))
    if rung.kind in helpers.REPEAT_KINDS:
        if rung.n <= 3000:
            want, ctr = compare(b, reads, DENSE, verify_modes=(0, 1), max_hits_ws=4_000_000)
            assert ctr["H"] > 100 * len(reads) and len(want) > 0
    else:
        assert ctr["H"] > 0 and (len(want) > 0 or rung.kind == "tinybins")  # (the test is not an empty one)


@pytest.mark.parametrize("name", WIDTH_RUNGS)
def test_forced_table_widths(built, name, monkeypatch):
    """MTSV_KMER_K: 1, 2, one less and one more than the upload picks by itself, 12 and 13 -- a table wider than the text,
    both parities of the ping-pong, the cap of the kept levels; MTSV_KMER_POS=0 and MTSV_KMER_LEVELS=0 once each.  Same
    hits, same n_seed_hits, and the info reports the width."""
    rung = helpers.RUNG_BY_NAME[name]
    b = built(rung)
    own = helpers.kmer_width_for(rung.n)
    rng = random.Random(rung.n + 4)
    reads = [r for _, r in helpers.position_probes(b.text)]
    if rung.n < 257:
        reads += [r for _, r in helpers.position_probes(b.text, width=8)] + tiny_extras(rng, b.text)
    else:  # some of them with an N in the table part of a seed
        reads += [helpers.substitute(rng, r, 1, alpha=b"N") for r in reads[::7]]
    param_sets = [dict(edit_rate=0.0), dict(edit_rate=0.0, seed_size=13, seed_interval=3)]
    if rung.n < 257:
        param_sets += list(SMALL_SEEDS)
    wants = []
    for over in param_sets:
        mp, op = both_params(**over)
        bases, off = helpers.reads_to_batch(reads)
        wants.append((mp,) + b.orc.bin_batch(bases, off, op, threads=8))
    settings = [("MTSV_KMER_K", str(k)) for k in sorted({1, 2, max(own - 1, 1), own, own + 1, 12, 13})]
    settings += [("MTSV_KMER_POS", "0"), ("MTSV_KMER_LEVELS", "0")]
    for var, val in settings:
        for flags in (M.DEV_DEFAULT, M.DEV_SAMPLED_SA_ONLY):
            ix2 = M.MGIndex.load(b.path)  # (to_device keeps what is resident when the flags are the same)
            monkeypatch.setenv(var, val)
            ix2.to_device(0, flags)
            monkeypatch.delenv(var)
            info = ix2.info()
            assert info["kmer_k"] == (int(val) if var == "MTSV_KMER_K" else own), (var, val, info)
            assert info["n"] == rung.n and info["sa_full"] == (0 if flags else 1)
            for mp, want, ctr in wants:
                got, st = run(ix2, reads, mp)
                assert_same_hits(got, want)
                assert_counters(st, ctr, not flags, (name, var, val, flags))
            ix2.close()
    assert sum(c["H"] for _, _, c in wants) > 0 or rung.n < 19


@pytest.mark.parametrize("rung", helpers.RUNGS, ids=repr)
def test_gpu_builder_writes_the_host_builders_bytes(built, rung, tmp_path):
    """mtsv_set_build_device(0): prefix doubling on the GPU writes the host builder's file, with the intervals (64, 32)
    and with the rung's own.  The composition rungs are its slow cases: ties that survive until h >= n."""
    b = built(rung)
    host = open(b.path, "rb").read()
    p = str(tmp_path / "gpu.idx")
    pairs = [(rung.occ_k, rung.sa_s)] + ([(64, 32)] if (rung.occ_k, rung.sa_s) != (64, 32) else [])
    for occ_k, sa_s in pairs:
        if (occ_k, sa_s) != (rung.occ_k, rung.sa_s):
            q = str(tmp_path / "host.idx")
            M.MGIndex.build(b.entries, occ_k, sa_s, threads=4).write(q)
            host = open(q, "rb").read()
        try:
            M.set_build_device(0)
            g = M.MGIndex.build(b.entries, occ_k, sa_s, threads=4)
        finally:
            M.set_build_device(-1)
        g.write(p)
        g.close()
        assert open(p, "rb").read() == host, (rung.name, occ_k, sa_s)
