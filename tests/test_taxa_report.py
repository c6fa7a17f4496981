"""-m gpu tests of the taxa report (k_report.hip, mtsv_batch_set_taxa_report / mtsv_batch_taxa_report, mtsv-binner
--report): per-TaxID read counts summed on the device.  The expected rows always come from the CPU oracle's hits through
the Python restatement of the semantics (taxa_report_ref.py), never from the device's own hits."""
import os
import random
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import taxa_report_ref as R
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
COLLAPSE = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")

PARAM_SETS = {
    "default": {},
    "stress": dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5),
    "dense": dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30),
    "loose": dict(edit_rate=0.3, max_candidates=40),
    "one_assignment": dict(max_assignments=1),
    "two_assignments": dict(max_assignments=2),
    "two_candidates": dict(max_candidates=2),
}


def both_params(**over):
    return M.default_params(**over), O.default_params(**{("seed_gap" if k == "seed_interval" else k): v for k, v in over.items()})


def index_taxa(path):
    """the distinct TaxIDs of an MG-index file: sequences (u64 length + bytes), then bins (u64 count, then gi u32, tax_id
    u32, start u64, end u64 each)"""
    raw = open(path, "rb").read()
    n = int.from_bytes(raw[:8], "little")
    at = 8 + n
    nb = int.from_bytes(raw[at:at + 8], "little")
    bins = np.frombuffer(raw, dtype=np.dtype([("gi", "<u4"), ("tax_id", "<u4"), ("start", "<u8"), ("end", "<u8")]), count=nb, offset=at + 8)
    return sorted(set(bins["tax_id"].tolist()))


def expected(orc, bases, off, op=None):
    want, _ = orc.bin_batch(bases, off, op or O.default_params(), threads=8)
    stats, total = R.classify_hits(want)
    return want, stats, total


def report(b, reset=False):
    rows, total, ms = b.taxa_report(reset=reset)
    assert list(rows["tax_id"]) == sorted(set(rows["tax_id"].tolist()))       # ascending, one row per TaxID
    assert all(any(int(r[c]) for c in R.COLS) for r in rows)                  # non-zero rows only
    assert ms >= 0
    return R.rows_dict(rows), total


def resident_report(ix, bases, off, mp=None, mode=None, **kw):
    b = M.Batch(ix, 0, max(len(off) - 1, 1), max(len(bases), 1), **kw)
    if mode is not None:
        b.set_verify_mode(mode)
    b.set_taxa_report(True)
    b.upload(bases, off)
    b.run(mp)
    got = report(b)
    st = b.stats()
    b.close()
    return got, st


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    ix = M.MGIndex.build_fasta(os.path.join(GOLD, "e2e_db.fasta"), threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "golden.idx")
    ix.write(p)
    ix.to_device(0)
    reads = [l.rstrip("\n").encode("latin-1") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    return ix, O.Index.read(p), reads, p


@pytest.fixture(scope="module")
def tricky(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.to_device(0)
    # reads of 150 and of 320 bases (the tiled path) in one batch
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=40, lengths=(150, 320))
    return ix, O.Index.read(p), reads, entries, gene, p


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    ix = M.MGIndex.synth(seed=5, n_taxa=24, gis_per_taxon=2, seq_len=20000)
    p = str(tmp_path_factory.mktemp("idx") / "synth.idx")
    ix.write(p)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=9, n_reads=100_000, read_len=150)
    orc = O.Index.read(p)
    want, stats, total = expected(orc, bases, off)
    return ix, bases, off, want, stats, total


@pytest.fixture(scope="module")
def many_taxa(tmp_path_factory):
    """more taxa than the dense tier holds: 4300 sequences of 220 bases, a TaxID each (some above 2^31)"""
    rng = random.Random(41)
    n = 4300
    assert n > 4095
    tax_ids = rng.sample(range(1, 1 << 32), n)
    entries = [(t, 10 + i, helpers.rnd_seq(rng, 220)) for i, t in enumerate(tax_ids)]
    # a segment shared by three of them, so that not every read is an only_hit
    shared = helpers.rnd_seq(rng, 120)
    for i in (5, 1700, 4200):
        t, g, s = entries[i]
        entries[i] = (t, g, s[:50] + shared + s[170:])
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "many.idx")
    ix.write(p)
    ix.to_device(0)
    assert len(index_taxa(p)) == n
    return ix, O.Index.read(p), entries, shared


def test_golden_database_gives_the_recorded_table(golden):
    ix, orc, reads, _ = golden
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(orc, bases, off)
    sums = tuple(sum(r[c] for r in stats.values()) for c in range(4))
    assert all(sums)                                          # all four categories are reached
    assert sums == (74, 24, 117, 358) and total == 140 and len(stats) == 12
    assert stats[2] == [38, 5, 10, 50] and stats[4000000000] == [5, 0, 0, 0]
    (got, got_total), _ = resident_report(ix, bases, off)
    assert got == stats and got_total == total
    # and through the formatter: the text mtsv-collapse --report writes from the golden results
    b = M.Batch(ix, 0, len(reads), len(bases))
    b.set_taxa_report(True)
    b.run_host(bases, off)
    rows, t, _ = b.taxa_report()
    b.close()
    assert R.parse_report(M.format_taxa_report(rows, t).decode()) == stats


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_adversarial_database_parameter_sets_and_verify_orders(tricky, pname, mode):
    """conserved gene in 8 taxa x 3 GIs (ties, one TaxID on both strands and in several GIs), tandem repeat, N runs;
    cut-offs of max_assignments / max_candidates change which hits a read keeps; reads of 150 and 320 bases"""
    ix, orc, reads, _, _, _ = tricky
    mp, op = both_params(**PARAM_SETS[pname])
    bases, off = helpers.reads_to_batch(reads)
    assert max(map(len, reads)) > 256
    want, stats, total = expected(orc, bases, off, op)
    assert total > 50
    (got, got_total), _ = resident_report(ix, bases, off, mp, mode)
    assert got == stats and got_total == total


def test_result_does_not_depend_on_how_the_reads_reach_the_device(synth):
    ix, bases, off, want, stats, total = synth
    n = len(off) - 1
    assert n >= 98304 and total > 0.8 * n and len(stats) == 24
    # (a) one resident upload + run: three lanes
    (got, got_total), st = resident_report(ix, bases, off)
    assert st["n_lanes"] == 3
    assert (got, got_total) == (stats, total)
    # (b) run_host
    b = M.Batch(ix, 0, n, len(bases))
    b.set_taxa_report(True)
    b.run_host(bases, off)
    assert report(b, reset=True) == (stats, total)
    # reset returned the accumulation and left zero
    assert report(b) == ({}, 0)
    # (c) run_host_parts in uneven pieces, an empty one among them
    cuts = [0, 7, 7, 40_001, 40_002, 77_777, n]
    parts = [(bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a]) for a, c in zip(cuts, cuts[1:])]
    b.run_host_parts(parts)
    assert report(b, reset=True) == (stats, total)
    # (d) two calls on halves without a reset in between: the report adds up over calls
    h = n // 2 + 13
    b.run_host(bases[: int(off[h])], off[: h + 1])
    first = report(b)
    assert first[1] < total
    b.run_host(bases[int(off[h]):], off[h:] - off[h])
    assert report(b) == (stats, total)
    # switched off, runs add nothing; the accumulation is kept and readable again once it is on
    b.set_taxa_report(False)
    b.run_host(bases[: int(off[1000])], off[:1001])
    with pytest.raises(M.MtsvError) as e:
        b.taxa_report()
    assert e.value.code == _lib.E_ARG
    b.set_taxa_report(True)
    assert report(b) == (stats, total)
    b.close()
    # (e) a workspace so small that the batch takes many passes
    b = M.Batch(ix, 0, 3000, 3000 * 150)
    b.set_taxa_report(True)
    b.run_host(bases, off)
    assert b.stats()["n_passes"] >= 30
    assert report(b) == (stats, total)
    b.close()
    # (f) one pass of more reads than the kernel's grid holds at a read per thread (workgroups of 16 wavefronts that
    # stride over the reads): the batch twelve times over in one lane; reads are independent, so every count is twelvefold
    # (the first pass of a workspace may run twice, the second time with a larger grid for its listed seeds, or in halves)
    k = 12
    kb = np.tile(bases, k)
    ko = np.concatenate([off[:-1] + i * off[-1] for i in range(k)] + [np.array([k * off[-1]], dtype=np.uint64)]).astype(np.uint64)
    assert k * n // 2 > 512 * 1024
    (got, got_total), st = resident_report(ix, kb, ko, lanes=1)
    assert st["n_lanes"] == 1 and st["n_passes"] <= 2
    assert (got, got_total) == ({t: [k * c for c in r] for t, r in stats.items()}, k * total)
    # a warm-up run of the workspace (mtsv_batch_reserve_host) is not part of the report
    b = M.Batch(ix, 0, n, len(bases), lanes=1)
    b.set_taxa_report(True)
    b.reserve_host(n, len(bases), warm_read_len=150)
    assert report(b) == ({}, 0)
    b.run_host(bases, off)
    assert report(b) == (stats, total)
    b.close()


def test_hit_workspace_overflow_counts_no_read_twice(tricky):
    """passes that are run again with fewer reads (seed-hit workspace too small) have not been counted"""
    ix, orc, reads, _, _, _ = tricky
    reads = [r for r in reads if len(r) <= 253]
    mp, op = both_params(seed_size=11, seed_interval=4, max_hits=100000, tune_max_hits=100000, min_seed=0.1)
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(orc, bases, off, op)
    (got, got_total), st = resident_report(ix, bases, off, mp, max_hits_ws=40000)
    assert st["n_passes"] > 1
    assert (got, got_total) == (stats, total)
    (got, got_total), st = resident_report(ix, bases, off, mp, max_hits_ws=64)
    assert st["n_passes"] > 100
    assert (got, got_total) == (stats, total)


def test_tiers_at_their_edges(tricky, many_taxa, monkeypatch, capfd):
    ix, orc, reads, entries, _, path = tricky
    n_taxa = len(index_taxa(path))
    assert 8 < n_taxa <= len({e[0] for e in entries})
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(orc, bases, off)
    monkeypatch.setenv("MTSV_TRACE", "1")
    tiers = {}
    for dense_max in (n_taxa - 1, n_taxa, n_taxa + 1, 1):
        monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", str(dense_max))
        capfd.readouterr()
        (got, got_total), _ = resident_report(ix, bases, off)
        err = capfd.readouterr().err
        assert f"[report] {n_taxa} taxa" in err
        tiers[dense_max] = "dense" if "dense tier" in err else "hashed" if "hashed tier" in err else None
        assert (got, got_total) == (stats, total), dense_max
    assert tiers == {n_taxa - 1: "hashed", n_taxa: "dense", n_taxa + 1: "dense", 1: "hashed"}
    # a hash table too small for the keys of a workgroup: what finds no place goes to the global counters directly
    monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", "1")
    monkeypatch.setenv("MTSV_REPORT_HASH_SLOTS", "16")
    (got, got_total), _ = resident_report(ix, bases, off)
    assert (got, got_total) == (stats, total)
    monkeypatch.delenv("MTSV_REPORT_DENSE_MAX")
    monkeypatch.delenv("MTSV_REPORT_HASH_SLOTS")
    # more taxa than the dense tier's real limit, no override
    mix, morc, mentries, shared = many_taxa
    rng = random.Random(3)
    mreads = []
    for i in range(6000):
        s = mentries[rng.randrange(len(mentries))][2]
        st = rng.randrange(0, len(s) - 100)
        r = helpers.mutate(rng, s[st:st + 100], rng.randrange(0, 6))
        mreads.append(r if i % 2 else helpers.revcomp(r))
    mreads += [helpers.mutate(rng, shared[:100], k % 5) for k in range(200)]
    mb, mo = helpers.reads_to_batch(mreads)
    mwant, mstats, mtotal = expected(morc, mb, mo)
    assert len(mstats) > 3000 and sum(r[2] + r[1] + r[3] for r in mstats.values()) > 100
    capfd.readouterr()
    (got, got_total), _ = resident_report(mix, mb, mo)
    assert "[report] 4300 taxa: hashed tier" in capfd.readouterr().err
    assert (got, got_total) == (mstats, mtotal)
    monkeypatch.setenv("MTSV_REPORT_HASH_SLOTS", "64")     # every workgroup overflows its table
    (got, got_total), _ = resident_report(mix, mb, mo)
    assert (got, got_total) == (mstats, mtotal)


def test_skewed_samples(tricky, many_taxa, monkeypatch):
    """every read on one taxon, and every read on the eight taxa of the conserved gene: the workgroups' LDS counters
    and their flush carry the whole sample (correctness of that path, not its speed)"""
    rng = random.Random(17)
    # one taxon of a many-taxa index (hashed tier)
    mix, morc, mentries, _ = many_taxa
    s = mentries[321][2]
    reads = [helpers.mutate(rng, s[st:st + 120], rng.randrange(0, 4)) for st in (rng.randrange(0, 100) for _ in range(20_000))]
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(morc, bases, off)
    assert list(stats) == [mentries[321][0]] and total > 19_000
    (got, got_total), _ = resident_report(mix, bases, off)
    assert (got, got_total) == (stats, total)
    # one taxon of a small index (dense tier): a sequence without the conserved gene
    tix, torc, _, tentries, gene, _ = tricky
    tax, _, s = next(e for e in tentries if e[0] == 17 and len(e[2]) > 1500)
    s = s.upper()
    reads = [helpers.mutate(rng, s[st:st + 150], rng.randrange(0, 4)) for st in (rng.randrange(0, len(s) - 150) for _ in range(8000))]
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(torc, bases, off)
    assert total > 7000 and stats[17][0] > 0.9 * total
    (got, got_total), _ = resident_report(tix, bases, off)
    assert (got, got_total) == (stats, total)
    # the eight taxa of the conserved gene: every read eight tied or near-tied taxa
    greads = []
    for i in range(6000):
        st = rng.randrange(0, len(gene) - 150)
        r = helpers.mutate(rng, gene[st:st + 150], rng.randrange(0, 3), b"ACGT")
        greads.append(r if i % 2 else helpers.revcomp(r))
    gb, go = helpers.reads_to_batch(greads)
    gwant, gstats, gtotal = expected(torc, gb, go)
    assert gtotal > 5500 and len(gstats) >= 8
    assert sum(r[2] for r in gstats.values()) > gtotal          # ties dominate
    for dense_max in (None, "1"):
        if dense_max:
            monkeypatch.setenv("MTSV_REPORT_DENSE_MAX", dense_max)
        (got, got_total), _ = resident_report(tix, gb, go)
        assert (got, got_total) == (gstats, gtotal)
        b = M.Batch(tix, 0, 1000, 1000 * 160)                   # and pass by pass through a small workspace
        b.set_taxa_report(True)
        b.run_host(gb, go)
        assert report(b) == (gstats, gtotal)
        b.close()


def test_reads_of_many_hits_are_classified_by_their_wavefront(tmp_path):
    """a segment planted in 90 taxa: every read of it carries a hit in each of them, more than one lane walks alone and
    more than one wavefront step; mixed with ordinary reads in the same wavefronts"""
    rng = random.Random(23)
    seg = helpers.rnd_seq(rng, 400)
    plants = []
    for t in range(90):
        copy = helpers.substitute(rng, seg, 2 * (t % 4))      # 0..6 substitutions: ties among the best and worse ones
        plants.append((copy, [(1000 + t, 5000 + t)]))
    background = [(7, 1, 3000), (8, 2, 3000), (9, 3, 3000)]
    entries = helpers.planted_db(rng, background, plants)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path / "planted.idx")
    ix.write(p)
    ix.to_device(0)
    orc = O.Index.read(p)
    reads = []
    for i in range(900):
        if i % 3 == 2:
            s = entries[i % 3][2]
            st = rng.randrange(0, len(s) - 150)
            reads.append(s[st:st + 150])
        else:
            st = rng.randrange(0, len(seg) - 150)
            r = helpers.mutate(rng, seg[st:st + 150], rng.randrange(0, 5), b"ACGT")
            reads.append(r if i % 2 else helpers.revcomp(r))
    bases, off = helpers.reads_to_batch(reads)
    want, stats, total = expected(orc, bases, off)
    per_read = np.bincount(want["read"].astype(np.int64))
    assert per_read.max() > 64 and (per_read > 16).sum() > 400       # more than one wavefront step per read
    for env in ({}, {"MTSV_REPORT_DENSE_MAX": "1"}):
        for k, v in env.items():
            os.environ[k] = v
        try:
            (got, got_total), _ = resident_report(ix, bases, off)
        finally:
            for k in env:
                del os.environ[k]
        assert (got, got_total) == (stats, total)


def test_off_is_off(tricky):
    ix, orc, reads, _, _, _ = tricky
    bases, off = helpers.reads_to_batch(reads)
    out = []
    for on in (False, True):
        b = M.Batch(ix, 0, len(reads), len(bases))
        if on:
            b.set_taxa_report(True)
        b.upload(bases, off)
        b.run()
        st = b.stats()
        out.append((b.download(), {k: v for k, v in st.items() if k.startswith("n_") or k in ("lf_steps", "window_bytes", "sw_cell_pairs", "myers_columns")}))
        if not on:
            with pytest.raises(M.MtsvError) as e:
                b.taxa_report()
            assert e.value.code == _lib.E_ARG
        b.close()
    assert_same_hits(out[1][0], out[0][0])
    assert out[1][1] == out[0][1]


def test_cli_report_equals_collapse_report_of_the_same_run(golden, tmp_path):
    _, _, reads, idx = golden
    fq = tmp_path / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i} desc\n{r.decode('latin-1')}\n+\n{'I' * len(r)}\n")
    for k, extra in enumerate(([], ["--devices", "0,0"], ["--batch-reads", "9"], ["--devices", "0,0,0", "--batch-reads", "7"])):
        res, rep = tmp_path / f"res{k}.txt", tmp_path / f"rep{k}.tsv"
        r = subprocess.run([BINNER, "--fastq", str(fq), "-i", idx, "-m", str(res), "--report", str(rep), *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out, crep = tmp_path / f"collapsed{k}.txt", tmp_path / f"crep{k}.tsv"
        assert subprocess.run([COLLAPSE, "-o", str(out), "--report", str(crep), str(res)], capture_output=True).returncode == 0
        assert rep.read_bytes() == crep.read_bytes()
        assert sorted(res.read_text().splitlines()) == sorted(open(os.path.join(GOLD, "e2e_default.results")).read().splitlines())
        assert R.parse_report(rep.read_text())[2] == [38, 5, 10, 50]
    # a report that cannot be written fails the run like a results file that cannot
    res = tmp_path / "res_bad.txt"
    r = subprocess.run([BINNER, "--fastq", str(fq), "-i", idx, "-m", str(res), "--report", str(tmp_path / "no_such_dir" / "rep.tsv")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 11
