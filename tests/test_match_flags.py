"""-m gpu tests of the match flags (k_match.hip, mtsv_batch_set_match_flags / mtsv_batch_match_flags, mtsv-binner --matched /
--unmatched): one bit per read, "the run returned a hit for it".  The expected flags always come from the CPU oracle's hits
(O.Index.bin_batch), never from the device's own hits, and every fixture is checked to hold matched and unmatched reads.

The oracle takes minutes on the 100 000 synthetic reads with the `dense` parameter set, so the synth fixture starts its
oracle runs on a thread of its own when it is created and the tests that need one wait for it; the tests are ordered so
that the expensive ones are asked for last."""
import concurrent.futures
import gzip
import os
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import partition_ref as P
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_partition_cpu import golden_records, write_input
from test_taxa_report import PARAM_SETS, both_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
PARTITION = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-partition")

MODES = {"with_hits": M.MATCH_WITH_HITS, "only": M.MATCH_ONLY}
N_SYNTH = 100_000          # the resident fixture
N_SYNTH_HOST = 100_003     # the host path: not a multiple of 64, three lanes (>= 98304)
CPUS = len(os.sched_getaffinity(0))


def presence(hits, n):
    p = np.zeros(n, dtype=bool)
    p[hits["read"].astype(np.int64)] = True
    return p


class Oracle:
    """the oracle's hits of one batch per parameter set, computed once (in the background when asked to)"""

    def __init__(self, orc, bases, off, threads=8):
        self.orc, self.bases, self.off, self.threads = orc, bases, off, threads
        self.jobs = {}
        self.pool = None  # (the synth fixture gives it one: its runs start in the background)

    def _run(self, pname):
        _, op = both_params(**PARAM_SETS[pname])
        want, _ = self.orc.bin_batch(self.bases, self.off, op, threads=self.threads)
        return want

    def hits(self, pname):
        if pname not in self.jobs:
            f = concurrent.futures.Future()
            f.set_result(self._run(pname))
            self.jobs[pname] = f
        return self.jobs[pname].result()

    def flags(self, pname):
        return presence(self.hits(pname), len(self.off) - 1)


def both_kinds(p):
    assert 0 < int(p.sum()) < len(p), "the fixture must hold matched and unmatched reads"
    return p


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    ix = M.MGIndex.synth(seed=5, n_taxa=24, gis_per_taxon=2, seq_len=20000)
    p = str(tmp_path_factory.mktemp("idx") / "synth.idx")
    ix.write(p)
    ix.to_device(0)
    # (read r is a function of (seed, r): the first 100 000 are the reads of test_taxa_report.py's fixture)
    bases, off = M.synth_reads(ix, seed=9, n_reads=N_SYNTH_HOST, read_len=150)
    orc = O.Index.read(p)
    host = Oracle(orc, bases, off, threads=max(4, min(16, CPUS)))
    resident = Oracle(orc, bases[: int(off[N_SYNTH])], off[: N_SYNTH + 1], threads=max(4, min(16, CPUS)))
    resident.pool = host.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    host.jobs["default"] = host.pool.submit(host._run, "default")
    for pname in sorted(PARAM_SETS, key=lambda k: (k == "dense", k)):      # the expensive one last
        if pname != "default":
            resident.jobs[pname] = resident.pool.submit(resident._run, pname)
    # the default set's hits on the first 100 000 reads are a prefix of those on all of them (hits are ordered by read)
    f = concurrent.futures.Future()
    resident.jobs["default"] = f
    host.jobs["default"].add_done_callback(
        lambda d: f.set_exception(d.exception()) if d.exception() else f.set_result(d.result()[d.result()["read"] < N_SYNTH]))
    yield ix, bases, off, host, resident
    host.pool.shutdown(wait=True, cancel_futures=True)


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    ix = M.MGIndex.build_fasta(os.path.join(GOLD, "e2e_db.fasta"), threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "golden.idx")
    ix.write(p)
    ix.to_device(0)
    reads = [l.rstrip("\n").encode("latin-1") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    bases, off = helpers.reads_to_batch(reads)
    return ix, bases, off, Oracle(O.Index.read(p), bases, off), p


@pytest.fixture(scope="module")
def tricky(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.to_device(0)
    # reads of 150 and of 320 bases (the tiled path) in one batch
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=40, lengths=(150, 320))
    assert max(map(len, reads)) > 256
    bases, off = helpers.reads_to_batch(reads)
    return ix, bases, off, Oracle(O.Index.read(p), bases, off)


def check_flags(b, want_flags, what=""):
    got, n_matched = b.match_flags()
    assert len(got) == len(want_flags), what
    bad = np.nonzero(got != want_flags)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], want_flags[bad[:10]])
    assert n_matched == int(want_flags.sum()), what


# ---- the host path: streams that OR into the same words, passes that start anywhere ----

def cut_parts(bases, off, n, sizes):
    """the first n reads in parts whose sizes cycle through `sizes`"""
    parts, a, k = [], 0, 0
    while a < n:
        c = min(n, a + sizes[k % len(sizes)])
        parts.append((bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a]))
        a, k = c, k + 1
    return parts


@pytest.mark.parametrize("lanes", [0, 1], ids=["three_lanes", "one_lane"])
@pytest.mark.parametrize("mname", list(MODES))
def test_host_path_read_counts_and_parts_off_the_word_grid(synth, mname, lanes):
    ix, bases, off, host, _ = synth
    want_all = both_kinds(host.flags("default"))
    want_hits = host.hits("default")
    mp, _ = both_params()
    b = M.Batch(ix, 0, N_SYNTH_HOST, len(bases), lanes=lanes)
    b.set_match_flags(MODES[mname])

    def check(n, what):
        check_flags(b, want_all[:n], what)
        st = b.stats()
        got = b.download()
        if MODES[mname] == M.MATCH_ONLY:
            assert len(got) == 0 and st["n_hits"] == 0, what
        else:
            assert_same_hits(got, want_hits[want_hits["read"] < n])
        return st

    # the largest first: every later run must leave none of its bits behind
    for n in (N_SYNTH_HOST, 65, 63, 1):
        b.run_host(bases[: int(off[n])], off[: n + 1], mp)
        st = check(n, f"run_host of {n} reads")
        if n == N_SYNTH_HOST:
            assert st["n_lanes"] == (3 if lanes == 0 else 1)
    for n, sizes in ((N_SYNTH_HOST, (1, 64, 1000)), (N_SYNTH_HOST, (1000,)), (65, (1, 64)), (65, (64, 1)), (63, (1,)), (1, (1,))):
        b.run_host_parts(cut_parts(bases, off, n, sizes), mp)
        check(n, f"run_host_parts of {n} reads in parts of {sizes}")
    b.close()
    # a seed-hit workspace small enough to force several passes per range
    b = M.Batch(ix, 0, N_SYNTH_HOST, len(bases), max_hits_ws=150_000, lanes=lanes)
    b.set_match_flags(MODES[mname])
    b.run_host(bases, off, mp)
    st = check(N_SYNTH_HOST, "small hit workspace")
    assert st["n_passes"] > 1 and st["n_passes"] > st["n_lanes"]
    b.run_host_parts(cut_parts(bases, off, 20_001, (1, 64, 1000)), mp)
    check(20_001, "small hit workspace, parts")
    b.close()


def test_a_second_run_with_fewer_reads_leaves_no_bit_of_the_first(synth):
    ix, bases, off, host, _ = synth
    want = host.flags("default")
    b = M.Batch(ix, 0, N_SYNTH_HOST, len(bases))
    b.set_match_flags(M.MATCH_ONLY)
    flags, n_matched = b.match_flags()                       # no run yet
    assert len(flags) == 0 and n_matched == 0
    b.run_host(bases, off)
    check_flags(b, want)
    # reads 70 .. 199 alone: the bits of the first run's reads 0 .. 129 would show
    a, c = 70, 200
    assert not np.array_equal(want[a:c], want[: c - a])
    b.run_host(bases[int(off[a]):int(off[c])], off[a:c + 1] - off[a])
    check_flags(b, want[a:c])                                 # (match_flags() itself rejects bits at and above n_reads)
    # the resident path on the same workspace, fewer reads still
    b.upload(bases[: int(off[40])], off[:41])
    b.run()
    check_flags(b, want[:40])
    # an empty run
    b.run_host(bases[:0], off[:1])
    flags, n_matched = b.match_flags()
    assert len(flags) == 0 and n_matched == 0
    b.close()


def test_modes_and_errors(golden):
    ix, bases, off, orc, _ = golden
    want = both_kinds(orc.flags("default"))
    b = M.Batch(ix, 0, len(off) - 1, len(bases))
    with pytest.raises(M.MtsvError) as e:                     # off by default
        b.match_flags()
    assert e.value.code == _lib.E_ARG
    with pytest.raises(M.MtsvError) as e:
        b.set_match_flags(3)
    assert e.value.code == _lib.E_ARG
    # MATCH_ONLY and the taxa report exclude each other, whichever comes second
    b.set_match_flags(M.MATCH_ONLY)
    with pytest.raises(M.MtsvError) as e:
        b.set_taxa_report(True)
    assert e.value.code == _lib.E_ARG
    b.set_match_flags(M.MATCH_OFF)
    b.set_taxa_report(True)
    with pytest.raises(M.MtsvError) as e:
        b.set_match_flags(M.MATCH_ONLY)
    assert e.value.code == _lib.E_ARG
    # ... while MATCH_WITH_HITS and the report go together
    b.set_match_flags(M.MATCH_WITH_HITS)
    b.run_host(bases, off)
    check_flags(b, want)
    rows, total, _ = b.taxa_report()
    assert total == int(want.sum())
    assert_same_hits(b.download(), orc.hits("default"))
    # switched off again: runs as ever, and no flags to be had
    b.set_match_flags(M.MATCH_OFF)
    b.run_host(bases, off)
    assert_same_hits(b.download(), orc.hits("default"))
    with pytest.raises(M.MtsvError) as e:
        b.match_flags()
    assert e.value.code == _lib.E_ARG
    b.close()
    # the warm-up run of a workspace is nobody's run
    b = M.Batch(ix, 0, len(off) - 1, len(bases))
    b.set_match_flags(M.MATCH_ONLY)
    b.reserve_host(len(off) - 1, len(bases), warm_read_len=100)
    flags, n_matched = b.match_flags()
    assert len(flags) == 0 and n_matched == 0
    b.run_host(bases, off)
    check_flags(b, want)
    b.close()


# ---- mtsv-binner --matched / --unmatched ----

def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def cli_inputs(golden, tmp_path_factory):
    _, _, _, orc, idx = golden
    d = tmp_path_factory.mktemp("cli")
    want = both_kinds(orc.flags("default"))
    forms = {}
    for name, fastq, gz in (("fastq", True, False), ("fasta", False, False), ("fastq.gz", True, True)):
        recs, headers = golden_records(fastq)
        path = d / f"reads.{name}"
        write_input(path, recs, headers, fastq, gz)
        forms[name] = (path, fastq, recs)
    return idx, want, forms


@pytest.mark.parametrize("extra", [("--devices", "0"), ("--devices", "0,0", "--batch-reads", "9")], ids=["one_worker", "two_workers_small_batches"])
@pytest.mark.parametrize("form", ["fastq", "fasta", "fastq.gz"])
def test_cli_fused_outputs_equal_the_restatement_on_the_oracles_flags(cli_inputs, tmp_path, form, extra):
    idx, want, forms = cli_inputs
    path, fastq, recs = forms[form]
    want_m, want_u = P.partition_by_flags(recs, want, fastq)
    assert want_m and want_u
    kind = "--fastq" if fastq else "--fasta"
    m, u = tmp_path / "m", tmp_path / "u"
    # flags only: no results file
    r = run_binner(kind, path, "-i", idx, "--matched", m, "--unmatched", u, *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert m.read_bytes() == want_m and u.read_bytes() == want_u
    assert f"{int(want.sum())} matched" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["m", "u"]
    # one side alone
    only_u = tmp_path / "only_u"
    r = run_binner(kind, path, "-i", idx, "--unmatched", only_u, *extra)
    assert r.returncode == 0 and only_u.read_bytes() == want_u
    # with --results: the results file is what a run without the new flags writes, byte for byte
    res0, res1 = tmp_path / "res0.txt", tmp_path / "res1.txt"
    assert run_binner(kind, path, "-i", idx, "-m", res0, *extra).returncode == 0
    m2, u2 = tmp_path / "m2", tmp_path / "u2"
    r = run_binner(kind, path, "-i", idx, "-m", res1, "--matched", m2, "--unmatched", u2, *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert res1.read_bytes() == res0.read_bytes() and len(res0.read_bytes()) > 0
    assert m2.read_bytes() == want_m and u2.read_bytes() == want_u
    # ... and mtsv-partition makes the same files from it (the fixture's IDs are unique)
    m3, u3 = tmp_path / "m3", tmp_path / "u3"
    assert subprocess.run([PARTITION, "--results", res1, kind, path, "--matched", m3, "--unmatched", u3], capture_output=True).returncode == 0
    assert m3.read_bytes() == want_m and u3.read_bytes() == want_u


def test_cli_interactions(cli_inputs, tmp_path):
    idx, want, forms = cli_inputs
    path, fastq, recs = forms["fastq"]
    m, u = tmp_path / "m", tmp_path / "u"
    # an existing results file without --force-overwrite would be resumed: refused, nothing created
    res = tmp_path / "res.txt"
    res.write_text("r0:2=4\n")
    r = run_binner("--fastq", path, "-i", idx, "-m", res, "--matched", m, "--unmatched", u)
    assert r.returncode == 1 and "resume" in r.stderr
    assert not m.exists() and not u.exists() and res.read_text() == "r0:2=4\n"
    # with --force-overwrite it runs (and the workspaces are torn down one by one: MTSV_CLI_CLEAN_EXIT)
    r = run_binner("--fastq", path, "-i", idx, "-m", res, "--matched", m, "--unmatched", u, "--force-overwrite", env={"MTSV_CLI_CLEAN_EXIT": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    want_m, want_u = P.partition_by_flags(recs, want, fastq)
    assert m.read_bytes() == want_m and u.read_bytes() == want_u
    assert sorted(res.read_text().splitlines()) == sorted(open(os.path.join(GOLD, "e2e_default.results")).read().splitlines())
    r = run_binner("--fastq", path, "-i", idx, "--matched", m, env={"MTSV_CLI_CLEAN_EXIT": "1", "MTSV_CLI_WORKERS": "2"})
    assert r.returncode == 0 and m.read_bytes() == want_m
    # --read-offset 7: the first seven reads go to neither file
    off_m, off_u = P.partition_by_flags(recs[7:], want[7:], fastq)
    assert off_m != want_m or off_u != want_u
    r = run_binner("--fastq", path, "-i", idx, "--matched", m, "--unmatched", u, "--read-offset", "7")
    assert r.returncode == 0, r.stdout + r.stderr
    assert m.read_bytes() == off_m and u.read_bytes() == off_u
    # the irregular-input fallback (a wrapped FASTQ record sends the rest of the file to the serial reader) and the
    # serial reader from the start give the plain path's output
    wrapped = tmp_path / "wrapped.fastq"
    k = next(i for i, rec in enumerate(recs) if i > 20 and len(rec[2]) > 100)
    with open(wrapped, "wb") as f:
        for i, (rec, h) in enumerate(zip(recs, golden_records(True)[1])):
            rid, desc, seq, qual = rec
            if i == k:
                f.write(b"@" + h + b"\n" + seq[:50] + b"\n" + seq[50:] + b"\n+\n" + qual[:50] + b"\n" + qual[50:] + b"\n")
            else:
                f.write(b"@" + h + b"\n" + seq + b"\n+\n" + qual + b"\n")
    for env in ({"MTSV_INGEST_BLOCK": "4096"}, {"MTSV_SERIAL_INGEST": "1"}):
        r = run_binner("--fastq", wrapped, "-i", idx, "--matched", m, "--unmatched", u, "--batch-reads", "9", env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert m.read_bytes() == want_m and u.read_bytes() == want_u
    gz = tmp_path / "wrapped.fastq.gz"
    with gzip.open(gz, "wb") as f:
        f.write(wrapped.read_bytes())
    r = run_binner("--fastq", gz, "-i", idx, "--matched", m, "--unmatched", u)
    assert r.returncode == 0 and m.read_bytes() == want_m and u.read_bytes() == want_u


# ---- the resident path: every parameter set, both verify orders, both match modes, three fixtures ----

def resident_case(ix, bases, off, orc, pname, vmode, n=None):
    n = len(off) - 1 if n is None else n
    mp, _ = both_params(**PARAM_SETS[pname])
    want_hits = orc.hits(pname)
    want = both_kinds(presence(want_hits, n))
    for mname, mode in MODES.items():
        b = M.Batch(ix, 0, max(n, 1), max(len(bases), 1))
        b.set_verify_mode(vmode)
        b.set_match_flags(mode)
        b.upload(bases, off)
        b.run(mp)
        check_flags(b, want, (pname, vmode, mname))
        st = b.stats()
        got = b.download()
        if mode == M.MATCH_ONLY:
            assert len(got) == 0 and st["n_hits"] == 0
        else:
            assert_same_hits(got, want_hits)
            assert st["n_hits"] == len(want_hits)
        assert st["n_reads"] == n and st["n_candidates"] > 0
        b.close()


@pytest.mark.parametrize("vmode", [0, 1], ids=["reference_order", "edit_first"])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_resident_golden(golden, pname, vmode):
    ix, bases, off, orc, _ = golden
    resident_case(ix, bases, off, orc, pname, vmode)


@pytest.mark.parametrize("vmode", [0, 1], ids=["reference_order", "edit_first"])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_resident_tricky(tricky, pname, vmode):
    """cut-offs of max_assignments / max_candidates (`stress`, `one_assignment`, `two_candidates`) change which hits a strand
    keeps, never whether it keeps one: a wrong clamp of max_assignments in flags-only mode would show here"""
    ix, bases, off, orc = tricky
    resident_case(ix, bases, off, orc, pname, vmode)


def test_max_assignments_zero_keeps_the_first_hit(tricky):
    """the reference checks the limit after it has pushed a hit (index.rs:421-425): --max-assignments 0 still keeps one"""
    ix, bases, off, orc = tricky
    mp, op = both_params(max_assignments=0)
    want_hits, _ = orc.orc.bin_batch(bases, off, op, threads=8)
    want = both_kinds(presence(want_hits, len(off) - 1))
    for mode in MODES.values():
        b = M.Batch(ix, 0, len(off) - 1, len(bases))
        b.set_match_flags(mode)
        b.upload(bases, off)
        b.run(mp)
        check_flags(b, want)
        b.close()


@pytest.mark.parametrize("vmode", [0, 1], ids=["reference_order", "edit_first"])
@pytest.mark.parametrize("pname", sorted(PARAM_SETS, key=lambda k: (k == "dense", k != "default", k)))
def test_resident_synth(synth, pname, vmode):
    ix, bases, off, _, resident = synth
    assert N_SYNTH >= 98304                                   # three lanes
    resident_case(ix, resident.bases, resident.off, resident, pname, vmode)
