"""-m gpu tests of folding chunk runs on the GPU (k_fold.hip, mtsv_fold_*, mtsv-binner --fold-on-gpu): an accumulator of
assignment records in HBM that outlives the workspace and the index of the chunk whose run it took.

Expected values never come from the device: synthetic lists are folded by the restatement (fold_ref.py); runs are compared
with the collapse (assign_ref.py, grain_ref.py) of the CPU oracle's per-chunk hits merged by chunk_merge_ref.py, reports with
taxa_report_ref.classify_hits.  Every comparison is exact."""
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
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_assignment_grains import synth  # noqa: F401  (fixture: 65 536 reads, the oracle's hits, their long collapse)
from test_chunk_merge import cli, planted5, run_binner, run_sources, tricky3  # noqa: F401  (fixtures)
from test_read_chain import sub_batch_arrays

pytestmark = pytest.mark.gpu

GRAINS = {"taxid": F.TAXID, "long": F.LONG, "taxid_gi": F.TAXID_GI}
COLLAPSE = {F.TAXID: A.collapse, F.LONG: GR.collapse_long, F.TAXID_GI: GR.collapse_taxid_gi}
B31 = 1 << 31


def as_array(grain, recs):
    return A.as_array(recs, M.ASSIGN_DTYPE) if grain == F.TAXID else GR.as_array(recs, M.ASSIGN_GI_DTYPE)


def records_of(fold):
    if fold.grain == F.TAXID:
        return A.as_triples(fold.download())
    return GR.as_tuples(fold.download_gi())


def check_fold(fold, want, n_reads):
    """records, count, report and flags of the fold against the restatement of `want`"""
    assert records_of(fold) == want
    assert fold.count() == len(want)
    rows, total, ms = fold.taxa_report()
    assert list(rows["tax_id"]) == sorted(set(rows["tax_id"].tolist())) and ms >= 0
    assert (R.rows_dict(rows), total) == F.report(want)
    flags, n_matched = fold.match_flags()
    pres = F.flags(want, n_reads)
    assert len(flags) == n_reads and np.array_equal(flags, pres) and n_matched == int(pres.sum())


# ---- 1. synthetic lists through add_records ----

def hi(x):
    """monotone, and from 2 on with bit 31 set"""
    return x if x < 2 else x | B31


OFFSETS = (0, 1, 2, 0xFFFFFFFF)


def rec(grain, slot, edit, offset=0, bits=6):
    """the record of key number `slot` (keys ascend with their number; 2 ** bits keys per read) with the given value"""
    read, low = slot >> bits, slot & ((1 << bits) - 1)
    if grain == F.TAXID:
        return (read, hi(low), edit)
    if grain == F.TAXID_GI:
        return (read, hi(low >> 2), hi(low & 3), offset, edit)
    return (read, hi(low >> 4), hi((low >> 2) & 3), OFFSETS[low & 3], edit)


def make(grain, rng, slots, bits=6):
    return [rec(grain, s, rng.randrange(0, 6), rng.randrange(0, 4), bits) for s in sorted(slots)]


def sample_pair(rng, n_a, n_b):
    """two sets of key numbers that share about a third of the smaller one"""
    space = range(3 * (n_a + n_b) + 8)
    sa = set(rng.sample(space, n_a))
    common = set(rng.sample(sorted(sa), min(n_a, n_b) // 3)) if n_a else set()
    sb = set(common)
    while len(sb) < n_b:
        sb.add(rng.choice(space))
    return sa, sb


def synthetic_cases(grain):
    rng = random.Random(100 + grain)
    cases = {}
    for n_a, n_b in ((0, 0), (0, 5), (5, 0), (63, 1), (64, 64), (65, 63), (197, 125)):
        sa, sb = sample_pair(rng, n_a, n_b)
        cases[f"sizes_{n_a}_{n_b}"] = (make(grain, rng, sa), make(grain, rng, sb))
    cases["one_and_one_equal_keys"] = (make(grain, rng, [9]), make(grain, rng, [9]))
    cases["b_before_a"] = (make(grain, rng, range(300, 400)), make(grain, rng, range(0, 90)))
    cases["b_after_a"] = (make(grain, rng, range(0, 90)), make(grain, rng, range(300, 400)))
    cases["interleaved"] = (make(grain, rng, range(0, 400, 2)), make(grain, rng, range(1, 400, 2)))
    cases["all_keys_equal"] = (make(grain, rng, range(5, 400, 3)), make(grain, rng, range(5, 400, 3)))
    # an equal pair at merged positions (63, 64), and at (127, 128): the A record ends a tile of 64, its B partner begins the next
    cases["pair_across_63_64"] = (make(grain, rng, range(0, 64)), make(grain, rng, [63, 70, 71]))
    cases["pair_across_127_128"] = (make(grain, rng, list(range(0, 200, 2)) + list(range(300, 328))), make(grain, rng, [327, 400]))
    # ... and with B records on both sides of the edge
    cases["pair_across_63_64_mixed"] = (make(grain, rng, range(0, 96, 2)), make(grain, rng, list(range(1, 32, 2)) + [94, 95, 97]))
    # one read that owns five tiles of 64 and more
    cases["one_read_of_five_tiles"] = (make(grain, rng, range(1024 + 3, 1024 + 603, 3), bits=10), make(grain, rng, range(1024, 1024 + 540, 2), bits=10))
    if grain == F.TAXID_GI:  # equal edits: the smaller offset; a smaller edit whatever its offset; from either side
        cases["ties"] = ([(0, 7, 1, 9, 3), (0, 7, 2, 50, 2), (0, 7, 3, 1, 5), (1, B31, B31, 4, 3)],
                         [(0, 7, 1, 4, 3), (0, 7, 2, 1, 5), (0, 7, 3, 50, 2), (1, B31, B31, 9, 3)])
    else:
        cases["ties"] = ([rec(grain, 3, 4), rec(grain, 4, 1), rec(grain, 5, 2)], [rec(grain, 3, 4), rec(grain, 4, 2), rec(grain, 5, 1)])
    return cases


def test_synthetic_cases_hold_what_they_claim():
    for grain in GRAINS.values():
        cases = synthetic_cases(grain)
        for a, b in cases.values():
            assert F.is_list(grain, a) and F.is_list(grain, b)
        for name, at in (("pair_across_63_64", 63), ("pair_across_127_128", 127), ("pair_across_63_64_mixed", 63)):
            a, b = cases[name]
            seq = sorted([(F.split(grain, r)[0], 0) for r in a] + [(F.split(grain, r)[0], 1) for r in b])  # A first among equals
            assert seq[at][0] == seq[at + 1][0] and (seq[at][1], seq[at + 1][1]) == (0, 1), name
        a, b = cases["one_read_of_five_tiles"]
        assert {r[0] for r in a + b} == {1} and len(a) + len(b) > 5 * 64
        a, b = cases["all_keys_equal"]
        assert len(F.fold(grain, a, b)) == len(a) == len(b) and F.fold(grain, a, b) != a and F.fold(grain, a, b) != b
        assert any(r[1] >= B31 for a, b in cases.values() for r in a + b)
        if grain != F.TAXID:
            assert any(r[2] >= B31 for a, b in cases.values() for r in a + b)
    a, b = synthetic_cases(F.TAXID_GI)["ties"]
    assert F.fold(F.TAXID_GI, a, b) == [(0, 7, 1, 4, 3), (0, 7, 2, 50, 2), (0, 7, 3, 50, 2), (1, B31, B31, 4, 3)]


@pytest.mark.parametrize("tile", ["64", None], ids=["tile64", "default_tile"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_synthetic_lists_fold_as_the_restatement_says(gname, tile, monkeypatch, capfd):
    grain = GRAINS[gname]
    if tile:
        monkeypatch.setenv("MTSV_FOLD_TILE", tile)
    else:
        monkeypatch.delenv("MTSV_FOLD_TILE", raising=False)
    monkeypatch.setenv("MTSV_TRACE", "1")
    fold = M.Fold(0, grain)
    for name, (a, b) in synthetic_cases(grain).items():
        n_reads = max([r[0] for r in a + b] + [0]) + 3
        for first, second in ((a, b), (b, a)):
            fold.reset(n_reads)
            assert fold.add_records(as_array(grain, first)) >= 0.0
            check_fold(fold, F.fold(grain, first, []), n_reads)
            assert fold.add_records(as_array(grain, second)) >= 0.0
            check_fold(fold, F.fold(grain, a, b), n_reads)
    fold.close()
    tiles = set(re.findall(r"\[fold\] \d+ \+ \d+ records -> \d+ in \d+ tiles of (\d+)", capfd.readouterr().err))
    assert tiles == {tile or "1024"}                                          # MTSV_FOLD_TILE is read when the fold is created


@pytest.mark.parametrize("gname", list(GRAINS))
def test_chain_of_six_folds_grows_the_accumulator(gname, monkeypatch, capfd):
    grain = GRAINS[gname]
    monkeypatch.setenv("MTSV_TRACE", "1")
    rng = np.random.default_rng(7 + grain)
    bits = 8
    lists = []
    for k in range(6):
        slots = np.sort(rng.choice(400_000, 15_000, replace=False))
        edits, offs = rng.integers(0, 9, len(slots)), rng.integers(0, 5, len(slots))
        lists.append([rec(grain, int(s), int(e), int(o), bits) for s, e, o in zip(slots, edits, offs)])
    n_reads = (400_000 >> bits) + 1
    fold = M.Fold(0, grain, n_reads=n_reads)
    want = []
    for l in lists:
        fold.add_records(as_array(grain, l))
        want = F.fold(grain, want, l)
        assert fold.count() == len(want)
    assert len(want) > 1 << 16 and len(want) < sum(len(l) for l in lists)     # beyond the first capacity; keys were joined
    check_fold(fold, want, n_reads)
    fold.close()
    grown = re.findall(r"\[fold\] accumulator grown from (\d+) to (\d+) records", capfd.readouterr().err)
    assert len(grown) >= 2 and int(grown[-1][0]) == 1 << 16 and int(grown[-1][1]) >= len(want)


# ---- 2. through runs: one chunk resident at a time ----

def fold_chunks(fx, grain, order, fold):
    """chunk c built, made resident, run in ASSIGN_ONLY and folded; its workspace and index are closed before the next exists"""
    fold.reset(fx.n)
    for c in order:
        ix = M.MGIndex.build(fx.entries[c], threads=4)
        ix.to_device(0)
        b = M.Batch(ix, 0, fx.n, len(fx.bases))
        b.set_assignment_grain(grain)
        b.set_assignments(M.ASSIGN_ONLY)
        b.upload(fx.bases, fx.off)
        b.run()
        assert fold.add_run(b) >= 0.0
        b.close()
        ix.close()


@pytest.mark.parametrize("gname", list(GRAINS))
@pytest.mark.parametrize("which", ["tricky3", "planted5"])
def test_chunks_that_take_turns_give_the_collapse_of_the_merge(which, gname, request):
    fx = request.getfixturevalue(which)
    grain = GRAINS[gname]
    merged = fx.merged()
    want = COLLAPSE[grain](merged)
    assert len(want) > 0
    fold = M.Fold(0, grain)
    fold_chunks(fx, grain, range(fx.k), fold)
    check_fold(fold, want, fx.n)
    raw = (fold.download() if grain == F.TAXID else fold.download_gi()).tobytes()
    stats, total = R.classify_hits(merged)
    rows, got_total, _ = fold.taxa_report()
    assert (R.rows_dict(rows), got_total) == (stats, total)
    if which == "tricky3":
        assert total == 182
    flags, n_matched = fold.match_flags()
    pres = CM.presence(merged, fx.n)
    assert np.array_equal(flags, pres) and n_matched == int(pres.sum())
    # the reversed chunk order gives the same bytes
    fold_chunks(fx, grain, reversed(range(fx.k)), fold)
    assert (fold.download() if grain == F.TAXID else fold.download_gi()).tobytes() == raw
    check_fold(fold, want, fx.n)                                              # ... and the same report and flags
    fold.close()
    # ... and they are the collector's records after merge_runs on the same chunks, all resident
    srcs = run_sources(fx)
    dst = M.Batch(fx.ixs[0], 0, 64, 1 << 12)
    dst.set_assignment_grain(grain)
    dst.set_assignments(M.ASSIGN_ONLY)
    dst.merge_runs(srcs)
    got = dst.download_assignments()[0] if grain == F.TAXID else dst.download_assignments_gi()[0]
    assert got.tobytes() == raw
    # a merged collector is a source of a fold too
    f2 = M.Fold(0, grain, n_reads=fx.n)
    f2.add_run(dst)
    check_fold(f2, want, fx.n)                                                # its report has the TaxIDs of every chunk, not only of dst's index
    rows, got_total, _ = f2.taxa_report()
    assert (R.rows_dict(rows), got_total) == (stats, total)
    if which == "tricky3":
        assert any(t in R.rows_dict(rows) for t in fx.absent_from_0)
    for b in srcs + [dst]:
        b.close()
    f2.close()


# ---- 3. a source whose run left several segments ----

def test_run_of_two_lanes_is_gathered_before_it_is_folded(synth):  # noqa: F811
    ix, bases, off, hits, want = synth
    n = len(off) - 1
    assert n == 65_536                                                       # the smallest batch a workspace of two lanes splits
    b = M.Batch(ix, 0, n, len(bases), lanes=2)
    b.set_assignment_grain(M.GRAIN_LONG)
    b.set_assignments(M.ASSIGN_ONLY)
    b.upload(bases, off)
    b.run()
    assert b.stats()["n_lanes"] == 2
    half = [r for r in want if r[0] % 2 == 0]
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=n)
    fold.add_records(GR.as_array(half, M.ASSIGN_GI_DTYPE))
    fold.add_run(b)
    b.close()
    got = fold.download_gi()
    assert got.tobytes() == GR.as_array(want, M.ASSIGN_GI_DTYPE).tobytes()
    flags, n_matched = fold.match_flags()
    pres = CM.presence(hits, n)
    assert np.array_equal(flags, pres) and n_matched == int(pres.sum())
    rows, total, _ = fold.taxa_report()
    assert (R.rows_dict(rows), total) == R.classify_hits(hits)
    fold.close()


# ---- 4. chunks behind a filter ----

def test_folded_chunks_behind_a_filter_carry_the_callers_numbers(tricky3):  # noqa: F811
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
    local = CM.merge_hits([orc.bin_batch(sb, so, O.default_params(), threads=16)[0] for orc in fx.orcs])
    merged = local.copy()
    merged["read"] = surv[local["read"].astype(np.int64)]
    want = A.collapse(merged)
    assert len(want) > 0 and any(r[0] != i for i, r in enumerate(want))
    f = M.Batch(f_ix, 0, fx.n, len(fx.bases))
    f.set_match_flags(M.MATCH_ONLY)
    f.upload(fx.bases, fx.off)
    f.run()
    first = M.Batch(fx.ixs[0], 0, fx.n, len(fx.bases))
    kept, _, _ = first.take_reads(f, M.KEEP_UNMATCHED)
    assert kept == len(surv)
    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=fx.n)
    for c in range(fx.k):
        b = first if c == 0 else M.Batch(fx.ixs[c], 0, fx.n, len(fx.bases))
        if c:
            b.copy_reads(first)
        b.set_assignments(M.ASSIGN_ONLY)
        b.run()
        fold.add_run(b)
        if c:
            b.close()
    check_fold(fold, want, fx.n)                                              # records and flags in the caller's numbering
    flags, _ = fold.match_flags()
    assert np.array_equal(flags, CM.presence(merged, fx.n)) and not flags[~np.isin(np.arange(fx.n), surv)].any()
    for b in (first, f):
        b.close()
    fold.close()
    f_ix.close()


# ---- 5. refusals ----

def test_refusals_leave_the_fold_as_it_was(tricky3):  # noqa: F811
    fx = tricky3
    nb = len(fx.bases)
    parts = fx.parts()
    before = A.collapse(parts[0])

    def source(c, grain=M.GRAIN_TAXID, mode=M.ASSIGN_ONLY, run="resident"):
        b = M.Batch(fx.ixs[c], 0, fx.n, nb)
        b.set_assignment_grain(grain)
        b.set_assignments(mode)
        if run == "resident":
            b.upload(fx.bases, fx.off)
            b.run()
        elif run == "host":
            b.run_host(fx.bases, fx.off)
        elif run == "none":
            b.upload(fx.bases, fx.off)
        return b

    fold = M.Fold(0, M.GRAIN_TAXID, n_reads=fx.n)
    s0 = source(0)
    fold.add_run(s0)
    check_fold(fold, before, fx.n)
    rows, total, _ = fold.taxa_report()
    report_before = (R.rows_dict(rows), total)

    def refused(call, code=_lib.E_ARG):
        with pytest.raises(M.MtsvError) as e:
            call()
        assert e.value.code == code, e.value
        check_fold(fold, before, fx.n)
        rows, total, _ = fold.taxa_report()
        assert (R.rows_dict(rows), total) == report_before

    others = [source(1, grain=M.GRAIN_LONG), source(1, mode=M.ASSIGN_OFF), source(1, run="none"), source(1, run="host")]
    for b in others:                                                          # grain mismatch, assignments off, no run, a host batch
        refused(lambda: fold.add_run(b))
    good = A.collapse(parts[1])
    unsorted = [good[1], good[0]] + good[2:]
    refused(lambda: fold.add_records(A.as_array(unsorted, M.ASSIGN_DTYPE)))    # keys not ascending
    refused(lambda: fold.add_records(A.as_array([good[0], good[0]] + good[1:], M.ASSIGN_DTYPE)))  # a key twice
    refused(lambda: fold.add_records(A.as_array(good + [(fx.n, 5, 1)], M.ASSIGN_DTYPE)))          # read >= n_reads
    refused(lambda: fold.download_gi())                                        # the wrong download call
    wide = M.Fold(0, M.GRAIN_TAXID_GI, n_reads=fx.n)
    with pytest.raises(M.MtsvError) as e:
        wide.download()
    assert e.value.code == _lib.E_ARG
    gi = GR.collapse_taxid_gi(parts[1])
    dup_pair = [gi[0], (*gi[0][:3], gi[0][3] + 1, gi[0][4])] + gi[1:]          # the same (read, tax_id, gi) at another offset
    with pytest.raises(M.MtsvError) as e:
        wide.add_records(GR.as_array(dup_pair, M.ASSIGN_GI_DTYPE))
    assert e.value.code == _lib.E_ARG and wide.count() == 0
    long_fold = M.Fold(0, M.GRAIN_LONG, n_reads=fx.n)
    long_fold.add_records(GR.as_array(sorted(dup_pair), M.ASSIGN_GI_DTYPE))    # ... which is two keys of the long grain
    assert long_fold.count() == len(dup_pair)
    # after all of it the fold still accepts a run
    s1 = source(1)
    fold.add_run(s1)
    check_fold(fold, A.collapse(CM.merge_hits(parts[:2])), fx.n)
    for b in others + [s0, s1]:
        b.close()
    for f in (fold, wide, long_fold):
        f.close()


# ---- 6. the command line ----

FOLD_CLI_CASES = {
    "plain": ([], {}, False),
    "fold_reads_100": (["--fold-reads", "100"], {}, False),
    "batch_reads_64": (["--batch-reads", "64"], {}, False),
    "long": (["--output-format", "long"], {}, True),
    "clean_exit": ([], {"MTSV_CLI_CLEAN_EXIT": "1"}, False),
}


@pytest.mark.parametrize("case", list(FOLD_CLI_CASES))
def test_binner_fold_on_gpu(cli, case, tmp_path):  # noqa: F811
    fx, d, index, fq, recs = cli
    extra, env, long_fmt = FOLD_CLI_CASES[case]
    env = {**env, "MTSV_CLI_TIMING": "1"}
    names = ("res.txt", "rep.tsv", "m.fq", "u.fq")
    got = [tmp_path / ("fold_" + n) for n in names]
    ref = [tmp_path / ("merge_" + n) for n in names]
    for switch, (res, rep, m, u) in (("--fold-on-gpu", got), ("--merge-on-gpu", ref)):
        args = [a for a in extra if switch == "--fold-on-gpu" or a not in ("--fold-reads", "100")]
        r = run_binner("--fastq", fq, "-i", index, "-m", res, switch, "--report", rep, "--matched", m, "--unmatched", u, *args, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        if switch == "--fold-on-gpu":
            timing = re.search(r"\[cli fold timing\] super_batches (\d+) chunks (\d+) reads (\d+)", r.stderr)
            assert timing and (int(timing.group(2)), int(timing.group(3))) == (fx.k, fx.n)
            if case == "fold_reads_100":
                assert int(timing.group(1)) >= 3                                  # 237 reads, at most 100 a super-batch
            else:
                assert int(timing.group(1)) == 1
    for a, b in zip(got, ref):
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 0
    ids = [rc[0].decode() for rc in recs]
    assert got[0].read_text() == M.format_results(fx.merged(), ids, long_format=long_fmt)
    stats, total = R.classify_hits(fx.merged())
    assert R.parse_report(got[1].read_text()) == stats and total == 182
    assert got[2].read_bytes().count(b"\n+\n") == 182 and got[3].read_bytes().count(b"\n+\n") == 55
    if case == "plain":  # --matched / --unmatched without a results file
        m3, u3 = tmp_path / "m3.fq", tmp_path / "u3.fq"
        r = run_binner("--fastq", fq, "-i", index, "--fold-on-gpu", "--matched", m3, "--unmatched", u3)
        assert r.returncode == 0, r.stdout + r.stderr
        assert m3.read_bytes() == got[2].read_bytes() and u3.read_bytes() == got[3].read_bytes()
