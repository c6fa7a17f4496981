"""-m gpu tests of the result lines written on the device (k_text.hip, mtsv_fold_format_text, mtsv_batch_format_text,
mtsv-binner --text-on-gpu).

Expected text never comes from the device or from the code under test: it is assign_ref.text / grain_ref.text (pinned against
the host formatters by test_text_cpu.py and the existing suites) applied to the synthetic lists of text_cases.py, to their fold
by fold_ref.py, or to the collapse of the CPU oracle's hits.  Every comparison is exact."""
import random
import re

import numpy as np
import pytest

import assign_ref as A
import chunk_merge_ref as CM
import fold_ref as F
import grain_ref as GR
import helpers
import mtsv_tools_amd as M
import taxa_report_ref as R
import text_cases as T
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_assignment_grains import synth  # noqa: F401  (fixture: 65 536 reads, the oracle's hits, their long collapse)
from test_chunk_merge import cli, planted5, run_binner, run_sources, tricky3  # noqa: F401  (fixtures)
from test_fold import as_array, check_fold
from test_read_chain import sub_batch_arrays

pytestmark = pytest.mark.gpu

GRAINS = T.GRAINS
COLLAPSE = {F.TAXID: A.collapse, F.LONG: GR.collapse_long, F.TAXID_GI: GR.collapse_taxid_gi}


def ids_of(n):
    return [f"r{i}" for i in range(n)]


def raw(fold):
    return (fold.download() if fold.grain == F.TAXID else fold.download_gi()).tobytes()


# ---- 1. synthetic lists through the fold ----

@pytest.mark.parametrize("tile", ["64", None], ids=["tile64", "default_tile"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_synthetic_lists_give_the_text_of_the_restatement(gname, tile, monkeypatch, capfd):
    grain = GRAINS[gname]
    if tile:
        monkeypatch.setenv("MTSV_TEXT_TILE", tile)
    else:
        monkeypatch.delenv("MTSV_TEXT_TILE", raising=False)
    monkeypatch.setenv("MTSV_TRACE", "1")
    fold = M.Fold(0, grain)
    monkeypatch.setenv("MTSV_TEXT_TILE", "2")                                 # (read when the fold was created, not later)
    for name, c in T.cases(grain).items():
        n_reads = len(c.ids)
        fold.reset(n_reads)
        fold.add_records(as_array(grain, c.records))
        before = raw(fold)
        got, ms = fold.format_text(c.table)
        assert got == T.expected(grain, c), name
        assert ms >= 0.0
        assert raw(fold) == before                                            # the fold is not changed: records, report, flags
        check_fold(fold, c.records, n_reads)
        assert fold.format_text(c.table)[0] == got, name                      # a second call gives the same bytes
        assert fold.format_text(c.ids)[0] == got, name                        # ... and so does the table built from the IDs
        fold.add_records(as_array(grain, c.second))
        both = F.fold(grain, c.records, c.second)
        assert fold.format_text(c.table)[0] == T.text(grain, both, c.ids), name
        check_fold(fold, both, n_reads)
    fold.close()
    tiles = set(re.findall(r"\[text\] \d+ records -> \d+ bytes in \d+ tiles of (\d+) ", capfd.readouterr().err))
    assert tiles == {tile or "1024"}


# ---- 2. refusals ----

def test_refusals_of_the_fold_leave_it_as_it_was():
    grain = F.TAXID
    c = T.cases(grain)["size_197"]
    n_reads = len(c.ids)
    fold = M.Fold(0, grain, n_reads=n_reads)
    fold.add_records(as_array(grain, c.records))
    want = T.expected(grain, c)
    blob, off = c.table
    for ids in (c.ids + ["one_more"], c.ids[:-1], (blob, off[:-1])):            # n_reads other than the reset's
        with pytest.raises(M.MtsvError) as e:
            fold.format_text(ids)
        assert e.value.code == _lib.E_ARG, e.value
        check_fold(fold, c.records, n_reads)
        assert fold.format_text(c.table)[0] == want
    r = c.records[5][0]
    assert r + 1 < n_reads
    for value in (int(off[-1]) + 7, int(off[r]) - 1 if off[r] else None):      # a slot that ends behind the ID bytes; one that ends before it begins
        if value is None:
            continue
        bad = off.copy()
        bad[r + 1] = value
        with pytest.raises(M.MtsvError) as e:
            fold.format_text((blob, bad))
        assert e.value.code == _lib.E_ARG, e.value
    assert fold.format_text(c.table)[0] == want
    check_fold(fold, c.records, n_reads)
    fold.close()


def test_refusals_of_a_workspace_leave_it_as_it_was(tricky3):  # noqa: F811
    fx = tricky3
    ids = ids_of(fx.n)
    want = T.text(F.TAXID, A.collapse(fx.parts()[0]), ids)
    assert len(want) > 0

    def refused(b, read_ids=ids):
        with pytest.raises(M.MtsvError) as e:
            b.format_text(read_ids)
        assert e.value.code == _lib.E_ARG, e.value

    b = M.Batch(fx.ixs[0], 0, fx.n, len(fx.bases))
    b.set_assignments(M.ASSIGN_ONLY)
    b.upload(fx.bases, fx.off)
    refused(b)                                                                # no run yet
    b.run()
    assert b.format_text(ids)[0] == want
    refused(b, ids[:100])                                                     # records of reads the ID table does not have
    assert b.format_text(ids)[0] == want
    assert A.as_triples(b.download_assignments()[0]) == A.collapse(fx.parts()[0])
    b.run_host(fx.bases, fx.off)
    refused(b)                                                                # a host batch: its records left range by range
    b.upload(fx.bases, fx.off)
    b.run()
    assert b.format_text(ids)[0] == want
    b.set_assignments(M.ASSIGN_OFF)
    b.run()
    refused(b)                                                                # assignments off
    b.set_assignments(M.ASSIGN_WITH_HITS)
    b.run()
    assert b.format_text(ids)[0] == want
    b.close()


# ---- 3. resident runs ----

_synth_want = {}


def synth_text(grain, hits, n):
    """the restatement's text of the collapse of the oracle's hits: computed once per grain, shared, never changed"""
    if grain not in _synth_want:
        _synth_want[grain] = T.text(grain, COLLAPSE[grain](hits), ids_of(n))
    return _synth_want[grain]


@pytest.mark.parametrize("mode", ["only", "with_hits"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_resident_run_gives_the_text_of_the_collapsed_oracle_hits(synth, gname, mode):  # noqa: F811
    ix, bases, off, hits, _ = synth
    grain = GRAINS[gname]
    n = len(off) - 1
    want = synth_text(grain, hits, n)
    assert want.count(b"\n") > 1024
    b = M.Batch(ix, 0, n, len(bases))
    b.set_assignment_grain(grain)
    b.set_assignments(M.ASSIGN_ONLY if mode == "only" else M.ASSIGN_WITH_HITS)
    b.upload(bases, off)
    b.run()
    got, ms = b.format_text(ids_of(n))
    assert got == want and ms >= 0.0
    assert b.format_text(ids_of(n))[0] == want
    b.close()


def test_run_of_two_lanes_is_gathered_before_its_text_is_written(synth):  # noqa: F811
    ix, bases, off, hits, _ = synth
    n = len(off) - 1
    b = M.Batch(ix, 0, n, len(bases), lanes=2)
    b.set_assignment_grain(M.GRAIN_LONG)
    b.set_assignments(M.ASSIGN_ONLY)
    b.upload(bases, off)
    b.run()
    assert b.stats()["n_lanes"] == 2
    assert b.format_text(ids_of(n))[0] == synth_text(F.LONG, hits, n)
    b.close()


# ---- 4. handed-over reads ----

def test_reads_handed_over_carry_the_callers_numbers_into_the_text(tricky3):  # noqa: F811
    fx = tricky3
    rng = random.Random(2024)
    every = [e for ch in fx.entries for e in ch]
    f_entries = every[::4] + [(700000 + k, 90000 + k, helpers.rnd_seq(rng, 2500)) for k in range(3)]
    f_ix = M.MGIndex.build(f_entries, threads=4)
    f_ix.to_device(0)
    f_want, _ = O.Index.build(f_entries).bin_batch(fx.bases, fx.off, O.default_params(), threads=16)
    surv = np.nonzero(~CM.presence(f_want, fx.n))[0]
    assert 0 < len(surv) < fx.n
    sb, so = sub_batch_arrays(fx.bases, fx.off, surv)
    local = fx.orcs[0].bin_batch(sb, so, O.default_params(), threads=16)[0]
    hits = local.copy()
    hits["read"] = surv[local["read"].astype(np.int64)]
    ids = [f"caller_{i}" for i in range(fx.n)]
    f = M.Batch(f_ix, 0, fx.n, len(fx.bases))
    f.set_match_flags(M.MATCH_ONLY)
    f.upload(fx.bases, fx.off)
    f.run()
    b = M.Batch(fx.ixs[0], 0, fx.n, len(fx.bases))
    kept, _, _ = b.take_reads(f, M.KEEP_UNMATCHED)
    assert kept == len(surv)
    for grain in GRAINS.values():
        want = COLLAPSE[grain](hits)
        assert len(want) > 0 and any(r[0] != i for i, r in enumerate(want))
        b.set_assignments(M.ASSIGN_OFF)
        b.set_assignment_grain(grain)
        b.set_assignments(M.ASSIGN_ONLY)
        b.run()
        assert b.format_text(ids)[0] == T.text(grain, want, ids)
    for x in (b, f):
        x.close()
    f_ix.close()


# ---- 5. merged runs ----

@pytest.mark.parametrize("which", ["tricky3", "planted5"])
def test_collector_gives_the_text_of_the_merged_oracle_hits(which, request):
    fx = request.getfixturevalue(which)
    ids = ids_of(fx.n)
    merged = CM.merge_hits(fx.parts())
    assert np.array_equal(merged, fx.merged())
    srcs = run_sources(fx)
    for grain in GRAINS.values():
        want = COLLAPSE[grain](merged)
        assert len(want) > 0
        dst = M.Batch(fx.ixs[0], 0, 64, 1 << 12)
        dst.set_assignment_grain(grain)
        dst.set_assignments(M.ASSIGN_ONLY)
        dst.merge_runs(srcs)
        got, ms = dst.format_text(ids)
        assert got == T.text(grain, want, ids) and ms >= 0.0
        dst.close()
    for b in srcs:
        b.close()


# ---- 6. the command line ----

@pytest.mark.parametrize("case", ["default", "long"])
def test_binner_text_on_gpu(cli, case, tmp_path):  # noqa: F811
    fx, d, index, fq, recs = cli
    extra = ["--fold-reads", "100"] + (["--output-format", "long"] if case == "long" else [])
    names = ("res.txt", "rep.tsv", "u.fq")
    got = [tmp_path / ("text_" + n) for n in names]
    ref = [tmp_path / ("host_" + n) for n in names]
    for flag, (res, rep, u) in ((["--text-on-gpu"], got), ([], ref)):
        r = run_binner("--fastq", fq, "-i", index, "-m", res, "--fold-on-gpu", *flag, "--report", rep, "--unmatched", u, *extra,
                       env={"MTSV_CLI_TIMING": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        timing = re.search(r"\[cli fold timing\] super_batches (\d+) chunks (\d+) reads (\d+)", r.stderr)
        assert timing and int(timing.group(1)) >= 2 and (int(timing.group(2)), int(timing.group(3))) == (fx.k, fx.n)
        assert ("[cli text timing]" in r.stderr) == bool(flag)
    ids = [rc[0].decode() for rc in recs]
    assert got[0].read_text() == M.format_results(fx.merged(), ids, long_format=case == "long") and len(got[0].read_bytes()) > 0
    for a, b in zip(got, ref):                                                 # the report and the unmatched reads as without the flag
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 0
    stats, total = R.classify_hits(fx.merged())
    assert R.parse_report(got[1].read_text()) == stats and total == 182
