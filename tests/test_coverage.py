"""-m gpu tests of coverage per reference (k_cover.hip, mtsv_coverage, mtsv-binner --coverage).

Records go in through mtsv_fold_add_records, so the kernels are tested without binning.  Expected values never come from the
device: they are cover_ref's -- a dict per reference with a bytearray of positions, and a loop over the records.  Every
comparison is exact.  The tile and tier settings (MTSV_COVER_TILE, MTSV_COVER_LANE_MAX) are read when an accumulator is
created, so every case makes its own under each of them; results must not depend on them."""
import collections
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import cover_cases as CC
import cover_ref as R
import helpers
import mtsv_tools_amd as M
import pack_ref
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
SETTINGS = {"tile64_lane0": ("64", "0"), "tile64_lane2": ("64", "2"), "defaults": (None, None)}
LANE_MAX = {"tile64_lane0": 0, "tile64_lane2": 2, "defaults": 8}
ALL = R.SLACK_ALL


def configure(monkeypatch, setting, trace=False):
    for name, value in zip(("MTSV_COVER_TILE", "MTSV_COVER_LANE_MAX"), SETTINGS[setting]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    if trace:
        monkeypatch.setenv("MTSV_TRACE", "1")
    else:
        monkeypatch.delenv("MTSV_TRACE", raising=False)


def accumulator(refs):
    c = M.Coverage(0)
    c.add_refs(*(zip(*refs) if refs else ((), (), ())))
    return c


def load(recs, n_reads):
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=n_reads)
    fold.add_records(CC.as_array(recs, M.ASSIGN_GI_DTYPE))
    return fold


def same_rows(c, want):
    got = R.as_tuples(c.rows()[0])
    if got != want:
        bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b][:5]
        raise AssertionError((len(got), len(want), [(got[k], want[k]) for k in bad]))


def add(c, recs, read_len, slack=0):
    """add_fold of a fold that holds recs; the fold is byte for byte what it was"""
    fold = load(recs, len(read_len))
    before = (fold.count(), fold.download_gi().tobytes())
    ms = c.add_fold(fold, read_len, slack)
    assert (fold.count(), fold.download_gi().tobytes()) == before and ms >= 0
    fold.close()
    return ms


def run_case(refs, folds, slack=0):
    c = accumulator(refs)
    for recs, read_len in folds:
        add(c, recs, read_len, slack)
    want = R.rows_of(refs, folds, slack)
    same_rows(c, want)
    same_rows(c, want)                                                                  # rows changes nothing
    assert M.format_coverage_report(c.rows()[0]) == R.report(want)
    c.close()
    return {(r[0], r[1]): r for r in want}


# ---- 1. edges ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_edges(setting, monkeypatch):
    configure(monkeypatch, setting)
    refs, folds = CC.edges()
    want = run_case(refs, folds)
    assert want[(5, 6)][3:] == (10, 10, 64 + 128 + 2 + 63 + 1 + 1 + 130 + 520 + 7 + 1, want[(5, 6)][6])
    assert want[(6, 1)][3:] == (2, 2, 6, 5) and want[(6, 2)][3:] == (0, 0, 0, 0)        # no bit leaks into the next reference
    assert want[(5, 5)][3:] == (2, 2, 1, 1)                                             # a read of no base is an alignment
    assert want[(5, 1)][6] == 1 and want[(CC.BIG, 7)][6] == 300 and want[(7, 1)][2:] == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_an_empty_fold_and_a_fold_of_no_reads(setting, monkeypatch):
    configure(monkeypatch, setting)
    refs = CC.EDGE_REFS
    c = accumulator(refs)
    for n_reads in (10, 0):
        fold = M.Fold(0, M.GRAIN_LONG, n_reads=n_reads)
        assert c.add_fold(fold, np.full(n_reads, 100, dtype=np.uint32)) == 0
        fold.close()
        rows, ms = c.rows()
        assert R.as_tuples(rows) == [(t, g, n, 0, 0, 0, 0) for t, g, n in sorted(refs)] and ms == 0
    with pytest.raises(M.MtsvError) as e:                                               # the first add_fold has come: the table is fixed
        c.add_refs([1], [1], [1])
    assert e.value.code == _lib.E_ARG
    c.add_refs(*zip(*refs))
    c.reset()
    c.add_refs([1], [1], [1])
    assert R.as_tuples(c.rows()[0]) == [(1, 1, 1, 0, 0, 0, 0)] + [(t, g, n, 0, 0, 0, 0) for t, g, n in sorted(refs)]
    c.close()
    empty = M.Coverage(0)                                                               # a table of no reference
    assert len(empty.rows()[0]) == 0 and M.format_coverage_report(empty.rows()[0]) == R.HEADER.encode()
    empty.close()


# ---- 2. slack ----

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("slack", [0, 1, 2, ALL])
def test_slack(slack, setting, monkeypatch):
    configure(monkeypatch, setting)
    refs, folds = CC.slack()
    want = run_case(refs, folds, slack)
    reads_alignments = {0: [(2, 2), (0, 0)], 1: [(2, 3), (1, 1)], 2: [(2, 3), (2, 2)], ALL: [(2, 4), (2, 4)]}[slack]
    assert [want[(10, g)][3:5] for g in (1, 2)] == reads_alignments                     # a run counts once, or not at all


# ---- 3. tiers ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_tiers(setting, monkeypatch, capfd):
    configure(monkeypatch, setting, trace=True)
    refs, folds, spans = CC.tiers()
    capfd.readouterr()
    run_case(refs, folds)
    line = re.search(r"\[cover\] .* (\d+) counted .* (\d+) on the work list", capfd.readouterr().err)
    assert line, "no [cover] line"
    assert int(line.group(1)) == len(spans)
    assert int(line.group(2)) == sum(1 for w in spans if w > LANE_MAX[setting])


# ---- 4. popcount tiles ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_popcount_tiles(setting, monkeypatch):
    configure(monkeypatch, setting)
    refs, folds = CC.pop_tiles()
    want = run_case(refs, folds)
    assert want[(31, 1)][6] > 5000 and sum(1 for k, r in want.items() if k[0] == 30 and r[6]) > 100


# ---- 5. hot locus ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_hot_locus(setting, monkeypatch):
    configure(monkeypatch, setting)
    refs, folds = CC.hot_locus()
    want = run_case(refs, folds)
    assert want[(40, 1)][3:] == (5000, 5000, 5000 * 150, 150)


# ---- 6. accumulation ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_accumulation_and_reset(setting, monkeypatch):
    configure(monkeypatch, setting)
    rng = random.Random(21)
    refs = CC.random_refs(rng, 60)
    a, b = CC.random_fold(rng, refs, 300), CC.random_fold(rng, refs, 200)
    c = accumulator(refs)
    add(c, *a, slack=1)
    same_rows(c, R.rows_of(refs, [a], 1))
    add(c, *b, slack=1)
    same_rows(c, R.rows_of(refs, [a, b], 1))                                            # rows in between changed nothing
    c.reset()
    same_rows(c, R.rows_of(refs, [], 1))
    add(c, *b, slack=1)
    same_rows(c, R.rows_of(refs, [b], 1))                                               # as on a fresh accumulator
    c.close()


# ---- 7. random ----

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("slack", [0, 1, ALL])
def test_random(slack, setting, monkeypatch):
    configure(monkeypatch, setting)
    refs, folds = CC.random_case()
    assert len(folds[0][0]) > 8000 and len(refs) == 300
    want = run_case(refs, folds, slack)
    assert sum(1 for r in want.values() if r[4]) > 100


# ---- 8. refusals ----

@pytest.mark.parametrize("setting", list(SETTINGS))
def test_refusals_leave_the_accumulator_as_it_was(setting, monkeypatch):
    configure(monkeypatch, setting)
    L = M.lib()
    refs = [(5, 1, 100), (5, 2, 200), (9, 1, 64)]
    good = [(0, 5, 1, 10, 0), (1, 5, 2, 150, 1), (2, 9, 1, 63, 0)]
    read_len = np.array([50, 100, 10, 7], dtype=np.uint32)
    c = accumulator(refs)
    add(c, good, read_len)
    want = R.rows_of(refs, [(good, read_len)])
    same_rows(c, want)
    folds = {
        "narrow": M.Fold(0, M.GRAIN_TAXID, n_reads=4),
        "gi": M.Fold(0, M.GRAIN_TAXID_GI, n_reads=4),
        "good": load(good, 4),
        "unknown": load(good + [(3, 5, 3, 0, 0)], 4),
        "beyond": load(good + [(3, 5, 1, 100, 0)], 4),
        "both": load([(0, 5, 1, 10, 0), (0, 8, 1, 10, 0), (1, 9, 1, 64, 3)], 4),
    }
    p_len = read_len.ctypes.data

    def refused(ch, fh, lens, n_reads, code=_lib.E_ARG):
        rc = L.mtsv_coverage_add_fold(ch, fh, lens, n_reads, 0, None)
        assert rc == code, (rc, L.mtsv_last_error())
        msg = L.mtsv_last_error().decode()
        same_rows(c, want)
        return msg

    assert "MTSV_GRAIN_LONG" in refused(c.h, folds["narrow"].h, p_len, 4)
    assert "MTSV_GRAIN_LONG" in refused(c.h, folds["gi"].h, p_len, 4)
    for n_reads in (3, 5):
        assert "reads" in refused(c.h, folds["good"].h, p_len, n_reads)                 # not the fold's n_reads
    refused(None, folds["good"].h, p_len, 4)
    refused(c.h, None, p_len, 4)
    refused(c.h, folds["good"].h, None, 4)
    assert "(tax_id 5, gi 3)" in refused(c.h, folds["unknown"].h, p_len, 4)             # named by its first record
    assert "(tax_id 5, gi 1) at offset 100" in refused(c.h, folds["beyond"].h, p_len, 4)
    msg = refused(c.h, folds["both"].h, p_len, 4)
    assert msg.startswith("arg: 1 records") and ", 1 lie" in msg and "record 1 (tax_id 8, gi 1)" in msg
    if M.device_count() > 1:
        far = M.Fold(1, M.GRAIN_LONG, n_reads=4)
        assert "device" in refused(c.h, far.h, p_len, 4)
        far.close()
    # the table is fixed: nothing new, nothing longer; what it holds already is accepted
    for new in ([(5, 3, 10)], [(5, 1, 101)], [(5, 1, 100), (1, 1, 1)]):
        with pytest.raises(M.MtsvError) as e:
            c.add_refs(*zip(*new))
        assert e.value.code == _lib.E_ARG and "fixed" in str(e.value)
        same_rows(c, want)
    c.add_refs(*zip(*refs))
    c.add_refs(*zip(*[(5, 1, 99), (9, 1, 0), (9, 1, 64)]))                              # shorter, and twice: nothing new
    same_rows(c, want)
    # the refused calls work once their cause is removed
    add(c, good, read_len)
    want = R.rows_of(refs, [(good, read_len)] * 2)
    same_rows(c, want)
    c.reset()
    c.add_refs(*zip(*[(5, 3, 10), (8, 1, 11), (9, 1, 65), (5, 1, 101)]))                 # after a reset the table grows again
    refs2 = refs + [(5, 3, 10), (8, 1, 11), (9, 1, 65), (5, 1, 101)]
    for name in ("unknown", "beyond", "both"):
        assert c.add_fold(folds[name], read_len) >= 0
    same_rows(c, R.rows_of(refs2, [([tuple(r) for r in folds[n].download_gi().tolist()], read_len) for n in ("unknown", "beyond", "both")]))
    # limits: MTSV_E_LIMIT, and the table stays
    d = accumulator(refs)
    for big in ([(1, 1, 2 ** 32)], [(1, k, 2 ** 32 - 1) for k in range(70)]):
        with pytest.raises(M.MtsvError) as e:
            d.add_refs(*zip(*big))
        assert e.value.code == _lib.E_LIMIT
    # a first add_fold that is refused leaves the table open
    rc = L.mtsv_coverage_add_fold(d.h, folds["unknown"].h, p_len, 4, 0, None)
    assert rc == _lib.E_ARG
    same_rows(d, R.rows_of(refs, []))
    d.add_refs([5], [3], [10])
    assert d.add_fold(folds["unknown"], read_len) >= 0
    same_rows(d, R.rows_of(refs + [(5, 3, 10)], [(good + [(3, 5, 3, 0, 0)], read_len)]))
    for x in (c, d, *folds.values()):
        x.close()


# ---- 9. end to end ----

def write_fastq(path, reads, ids):
    with open(path, "wb") as f:
        for r, i in zip(reads, ids):
            f.write(b"@" + i.encode() + b" some description\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("cover_e2e")
    chunks = []
    for c, seed in enumerate((5, 6)):
        ix = M.MGIndex.synth(seed=seed, n_taxa=8, gis_per_taxon=2, seq_len=20000)
        p = str(d / f"chunk{c}.idx")
        ix.write(p)
        ix.to_device(0)
        chunks.append((ix, p))
    files = [pack_ref.IndexFile(p) for _, p in chunks]
    b, s, e, reads = CC.e2e_reads(files[0])
    ids = [f"frag{k // 2}/{1 + k % 2}" for k in range(len(reads))]                       # mates by name, for --interleaved
    fq = d / "reads.fastq"
    write_fastq(fq, reads, ids)
    bases, off = helpers.reads_to_batch(reads)
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=len(reads))
    for ix, _ in chunks:
        batch = M.Batch(ix, 0, len(reads), len(bases), lanes=1)
        batch.set_assignment_grain(M.GRAIN_LONG)
        batch.set_assignments(M.ASSIGN_ONLY)
        batch.upload(bases, off)
        batch.run()
        fold.add_run(batch)
        batch.close()
    recs = [tuple(r) for r in fold.download_gi().tolist()]
    refs = [(x[1], x[0], x[3] - x[2]) for f in files for x in f.bins]
    read_len = [len(r) for r in reads]
    E = collections.namedtuple("E", "dir index fq reads fold recs refs read_len chunks stretch others")
    yield E(d, ",".join(p for _, p in chunks), fq, reads, fold, recs, refs, read_len, [ix for ix, _ in chunks], (b, s, e),
            CC.untouched_refs(files[0], b))
    fold.close()


_WANT = {}


def wanted(e2e, slack):
    if slack not in _WANT:
        _WANT[slack] = R.rows_of(e2e.refs, [(e2e.recs, e2e.read_len)], slack)
    return _WANT[slack]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_library_path_on_binned_reads(setting, e2e, monkeypatch):
    configure(monkeypatch, setting)
    c = M.Coverage(0)
    for ix in e2e.chunks:
        c.add_index(ix)
    before = e2e.fold.download_gi().tobytes()
    c.add_fold(e2e.fold, e2e.read_len)
    assert e2e.fold.download_gi().tobytes() == before
    want = wanted(e2e, 0)
    same_rows(c, want)
    assert len(want) == 32 and len(e2e.recs) > len(e2e.reads) // 2
    CC.condition(R.as_tuples(c.rows()[0]), *e2e.stretch, e2e.others)
    c.close()


def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


def settings_env(setting):
    """the two knobs as the binner's accumulator reads them"""
    return {name: value for name, value in zip(("MTSV_COVER_TILE", "MTSV_COVER_LANE_MAX"), SETTINGS[setting]) if value is not None}


VARIANTS = {
    "plain": ([], 0),
    "dedup_text_on_gpu": (["--dedup", "--text-on-gpu"], 0),
    "many_super_batches": (["--batch-reads", "63", "--fold-reads", "190"], 0),
    "slack_all": (["--coverage-slack", "all"], ALL),
}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_binner_coverage_writes_the_text_of_the_restatement(variant, setting, e2e, tmp_path, monkeypatch):
    configure(monkeypatch, setting)
    flags, slack = VARIANTS[variant]
    res, cov = tmp_path / "res.txt", tmp_path / "cov.tsv"
    r = run_binner("--fastq", e2e.fq, "-i", e2e.index, "-m", res, "--fold-on-gpu", "--output-format", "long", "--coverage", cov, *flags,
                   env={"MTSV_CLI_TIMING": "1", **settings_env(setting)})
    assert r.returncode == 0, r.stdout + r.stderr
    want = wanted(e2e, slack)
    assert cov.read_bytes() == R.report(want) and sum(1 for row in want if row[4]) >= 2
    assert re.search(r"\[cli coverage timing\] coverage device [\d.]+ ms", r.stderr)
    if variant == "many_super_batches":
        assert int(re.search(r"super_batches (\d+)", r.stderr).group(1)) > 2


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_binner_coverage_of_pairs_is_that_of_their_reads(setting, e2e, tmp_path, monkeypatch):
    configure(monkeypatch, setting)
    res, cov = tmp_path / "res.txt", tmp_path / "cov.tsv"
    r = run_binner("--fastq", e2e.fq, "-i", e2e.index, "-m", res, "--fold-on-gpu", "--interleaved", "--pair-mode", "proper", "--coverage", cov,
                   env=settings_env(setting))
    assert r.returncode == 0, r.stdout + r.stderr
    assert cov.read_bytes() == R.report(wanted(e2e, 0))
