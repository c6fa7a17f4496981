"""-m gpu tests of the pair join (k_pair.hip, mtsv_fold_pair, mtsv-binner --interleaved).

Records go in through mtsv_fold_add_records, so the kernels are tested without binning.  Expected values never come from the
device: they are pair_ref's -- a dict per pair, a double loop for PROPER -- of the records the fold holds.  Every comparison is
exact.  check() compares the output fold's records and the stats, and that the source fold is byte for byte what it was; the
tile and tier settings (MTSV_PAIR_TILE, MTSV_PAIR_LANE_MAX) are read when a fold is created, so every case makes its own."""
import collections
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import assign_ref as A
import fold_ref as F
import helpers
import lca_ref as LR
import mtsv_tools_amd as M
import pack_ref
import pair_cases as PC
import pair_ref as R
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
FIXTURE = os.path.join(ROOT, "tests", "golden", "nodes_primates.dmp")
DT = (M.ASSIGN_DTYPE, M.ASSIGN_GI_DTYPE)
U32 = 2 ** 32 - 1
MODES = {"both": R.BOTH, "either": R.EITHER, "proper": R.PROPER}
SETTINGS = {"tile64_lane0": ("64", "0"), "tile64_lane3": ("64", "3"), "defaults": (None, None)}
# (mode, grain) as the library accepts them
COMBOS = [(m, g) for m in ("both", "either") for g in PC.GRAINS] + [("proper", "long")]
COMBO_IDS = [f"{m}-{g}" for m, g in COMBOS]
UNPAIRED = 5


def configure(monkeypatch, setting):
    for name, value in zip(("MTSV_PAIR_TILE", "MTSV_PAIR_LANE_MAX"), SETTINGS[setting]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def raw(fold):
    return (fold.download() if fold.grain == M.GRAIN_TAXID else fold.download_gi()).tobytes()


def triples(a):
    return list(zip(a["read"].tolist(), a["tax_id"].tolist(), a["edit"].tolist()))


def load(grain, n_reads, wide):
    """(a fold of the grain that holds the case, the records it holds)"""
    recs = PC.project(grain, wide)
    fold = M.Fold(0, grain, n_reads=n_reads)
    fold.add_records(PC.as_array(grain, recs, DT))
    return fold, recs


_WANT = {}


def wanted(key, mode, recs, max_insert, unpaired):
    """pair_ref's list, computed once per case (key), mode and parameters"""
    k = (key, mode, max_insert, unpaired)
    if k not in _WANT:
        _WANT[k] = R.pair(mode, recs, max_insert, unpaired)
    return _WANT[k]


def check(fold, recs, n_reads, mode, max_insert=0, unpaired=0, out=None, key=None):
    want = wanted(key, mode, recs, max_insert, unpaired) if key else R.pair(mode, recs, max_insert, unpaired)
    before = (fold.count(), raw(fold))
    own = out is None
    if own:
        out = M.Fold(0, M.GRAIN_TAXID)
    stats, ms = fold.pair(mode, max_insert, unpaired, out=out)
    assert (fold.count(), raw(fold)) == before and ms >= 0                              # f is unchanged
    got = triples(out.download())
    if got != want:
        bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b][:5]
        raise AssertionError((len(got), len(want), [(got[k], want[k]) for k in bad]))
    assert out.count() == len(want)
    assert stats == R.stats(recs, n_reads, want), (stats, R.stats(recs, n_reads, want))
    flags, matched = out.match_flags()
    assert len(flags) == n_reads // 2 and matched == stats["joined"]                    # as after mtsv_fold_reset(out, P)
    if own:
        out.close()
    return want


def run_case(name, mode, gname, n_reads, wide, max_insert=0):
    grain = PC.GRAINS[gname]
    fold, recs = load(grain, n_reads, wide)
    want = check(fold, recs, n_reads, MODES[mode], max_insert, UNPAIRED, key=(name, gname))
    fold.close()
    return want


# ---- 1. edges ----

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mode,gname", COMBOS, ids=COMBO_IDS)
def test_edges(mode, gname, setting, monkeypatch):
    configure(monkeypatch, setting)
    n_reads, wide = PC.edges()
    want = run_case("edges", mode, gname, n_reads, wide, max_insert=100)
    pairs = {p for p, _, _ in want}
    assert 0 in pairs and 7 in pairs and 1 not in pairs and 6 not in pairs              # the first and the last pair; empty pairs
    assert (2 in pairs) == (3 in pairs) == (mode == "either")                           # one mate only
    assert any(t >= 2 ** 31 for _, t, _ in want)
    if mode == "either":                                                                # mate 1's taxa below, between and above
        assert [t for p, t, _ in want if p == 4] == [5, 10, 15, 20, 25]
        assert [e for p, _, e in want if p == 4] == [0 + UNPAIRED, 1 + 3, 1 + UNPAIRED, 2 + 0, 2 + UNPAIRED]


@pytest.mark.parametrize("mode,gname", COMBOS, ids=COMBO_IDS)
def test_an_empty_fold_and_a_fold_of_no_reads(mode, gname):
    for n_reads in (10, 0):
        fold = M.Fold(0, PC.GRAINS[gname], n_reads=n_reads)
        out = M.Fold(0, M.GRAIN_TAXID, n_reads=3)
        out.add_records(PC.as_array(F.TAXID, [(1, 5, 5)], DT))
        stats, ms = fold.pair(MODES[mode], 100, UNPAIRED, out=out)
        assert stats == {"pairs": n_reads // 2, "both_mates_hit": 0, "one_mate_hit": 0, "joined": 0, "records": 0} and ms == 0
        assert out.count() == 0 and len(out.match_flags()[0]) == n_reads // 2
        assert out.format_text([f"p{k}" for k in range(n_reads // 2)])[0] == b""
        fold.close()
        out.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("max_insert", [0, 1, U32])
def test_offsets_at_both_ends_do_not_wrap(max_insert, setting, monkeypatch):
    configure(monkeypatch, setting)
    n_reads, wide = PC.offsets()
    want = run_case("offsets", "proper", "long", n_reads, wide, max_insert=max_insert)
    assert [p for p, _, _ in want] == {0: [3, 4], 1: [0, 3, 4], U32: [0, 1, 2, 3, 4]}[max_insert]


# ---- 2. tier and tile edges ----

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mode,gname", COMBOS, ids=COMBO_IDS)
def test_windows_at_the_edge_of_the_lane_tier(mode, gname, setting, monkeypatch, capfd):
    # windows of 0, 1, 3, 4, 16, 17 records by offset (PROPER) and by TaxID (BOTH / EITHER at the LONG grain, where the window
    # also holds the three records outside the offsets): at and one past MTSV_PAIR_LANE_MAX = 0, 3 and 16
    configure(monkeypatch, setting)
    monkeypatch.setenv("MTSV_TRACE", "1")
    n_reads, wide = PC.windows(sizes=(0, 1, 3, 4, 13, 14, 16, 17, 18))
    want = run_case("windows", mode, gname, n_reads, wide, max_insert=20)
    assert len(want) >= 16
    listed = int(re.search(r"\[pair\] .* (\d+) on the work list", capfd.readouterr().err).group(1))
    lane_max = int(SETTINGS[setting][1] or 16)
    sizes = [w if mode == "proper" else w + 3 if gname == "long" else 2 if gname == "taxid_gi" else 1 for w in (0, 1, 3, 4, 13, 14, 16, 17, 18) for _ in (0, 1)]
    assert listed == sum(1 for w in sizes if w > lane_max)


@pytest.mark.parametrize("setting", ["tile64_lane3", "defaults"])
@pytest.mark.parametrize("mode,gname", COMBOS, ids=COMBO_IDS)
def test_runs_and_mates_that_straddle_tiles(mode, gname, setting, monkeypatch):
    configure(monkeypatch, setting)
    n_reads, wide = PC.straddle()
    want = run_case("straddle", mode, gname, n_reads, wide, max_insert=40)
    assert [t for p, t, _ in want if p == 0] == ([1, 2, 3] if mode == "either" else [1] if mode == "proper" else [1, 2])


@pytest.mark.parametrize("setting", ["tile64_lane3", "defaults"])
@pytest.mark.parametrize("mode", ["proper", "both"])
def test_a_heavy_pair_among_ordinary_ones(mode, setting, monkeypatch, capfd):
    configure(monkeypatch, setting)
    monkeypatch.setenv("MTSV_TRACE", "1")
    n_reads, wide = PC.heavy()
    want = run_case("heavy", mode, "long", n_reads, wide, max_insert=500)
    listed = int(re.search(r"\[pair\] .* (\d+) on the work list", capfd.readouterr().err).group(1))
    assert listed >= (2048 if mode == "proper" else 1)                                  # every record of the heavy mate 0, or its head
    assert (40, 4, 3) in want and ((40, 9, 0) in want) == (mode == "both")              # (2 + 1: the smallest sum in reach)


# ---- 3. random ----

@pytest.fixture(scope="module")
def random_case():
    return PC.random_pairs(random.Random(17), n_pairs=2000)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mode,gname", COMBOS, ids=COMBO_IDS)
def test_random_pairs(mode, gname, setting, monkeypatch, random_case):
    configure(monkeypatch, setting)
    n_reads, wide = random_case
    grain = PC.GRAINS[gname]
    fold, recs = load(grain, n_reads, wide)
    assert len(recs) > 8000
    for max_insert in ((0, 1, 300, U32) if mode == "proper" else (0,)):
        want = check(fold, recs, n_reads, MODES[mode], max_insert, UNPAIRED, key=("random", gname))
        assert len({p for p, _, _ in want}) > ({0: 50, 1: 100, 300: 200, U32: 500}[max_insert] if mode == "proper" else 800)
    fold.close()


# ---- 4. out is a full fold ----

@pytest.mark.parametrize("mode", list(MODES))
def test_everything_a_fold_offers_works_on_the_pair_fold(mode, monkeypatch, tmp_path):
    configure(monkeypatch, "tile64_lane3")
    tx_ref, tx_lib = LR.Taxonomy(open(FIXTURE).read()), M.Taxonomy(FIXTURE)
    rng = random.Random(23)
    pool = rng.sample(tx_ref.listed, 12) + [77]
    n_pairs = 300
    wide = []
    for read in range(2 * n_pairs):
        for t in rng.sample(pool, rng.choice((0, 1, 1, 2, 3, 6))):
            for gi in range(1, rng.randrange(1, 3) + 1):
                wide.append((read, t, gi, rng.randrange(2000), rng.randrange(5)))
    fold, recs = load(F.LONG, 2 * n_pairs, wide)
    out = M.Fold(0, M.GRAIN_TAXID)
    want = check(fold, recs, 2 * n_pairs, MODES[mode], 600, UNPAIRED, out=out)
    assert len(want) > (50 if mode == "proper" else 100)                                # (the case is not empty in any mode)
    ids = [f"pair_{k}" for k in range(n_pairs)]
    assert out.format_text(ids)[0] == A.text(want, ids).encode() == R.lines(want, ids)
    rows, total, _ = out.taxa_report()
    stats, reads = F.report(want)
    assert {int(r["tax_id"]): [int(r[c]) for c in ("only_hit", "only_best", "tied_best", "not_best")] for r in rows} == stats and total == reads
    flags, matched = out.match_flags()
    assert np.array_equal(flags, F.flags(want, n_pairs)) and matched == reads
    lca_out = M.Fold(0, M.GRAIN_TAXID)
    _, lca_total, _ = out.lca(tx_lib, 0, out=lca_out)
    assert triples(lca_out.download()) == LR.per_read(tx_ref, want, 0) and lca_total == reads
    for f in (fold, out, lca_out):
        f.close()


def test_an_output_fold_that_holds_more_and_one_that_must_grow(monkeypatch):
    configure(monkeypatch, "defaults")
    n = 70000                                                                           # pairs: above the first allocation of a fold
    wide = [(r, 3 + (r >> 1) % 4, 1, 10, r % 5) for r in range(2 * n)]
    fold, recs = load(F.TAXID, 2 * n, wide)
    small = M.Fold(0, M.GRAIN_TAXID, n_reads=2)
    small.add_records(PC.as_array(F.TAXID, [(1, 5, 5)], DT))
    stats, _ = fold.pair(M.PAIR_BOTH, out=small)
    got = small.download()
    assert stats["records"] == n == stats["joined"] and np.array_equal(got["read"], np.arange(n))
    assert np.array_equal(got["edit"], np.array([(2 * p) % 5 + (2 * p + 1) % 5 for p in range(n)], dtype=np.uint32))
    little, lrecs = load(F.TAXID, 4, [(0, 9, 1, 0, 1), (1, 9, 1, 0, 2)])
    check(little, lrecs, 4, R.BOTH, out=small)                                          # the same fold takes a shorter list
    for f in (fold, small, little):
        f.close()


# ---- 5. refusals ----

def test_refusals_leave_the_output_fold_as_it_was():
    L = M.lib()
    even, _ = load(F.LONG, 6, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2)])
    narrow_f, _ = load(F.TAXID, 6, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2)])
    gi_f, _ = load(F.TAXID_GI, 6, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2)])
    odd, _ = load(F.LONG, 5, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2)])
    big_edit, _ = load(F.LONG, 6, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2 ** 31), (4, 5, 1, 20, U32)])
    wide_out, _ = load(F.LONG, 4, [(2, 5, 1, 1, 5)])
    out, _ = load(F.TAXID, 4, [(2, 5, 1, 1, 5), (3, 6, 1, 1, 0)])
    folds = (even, narrow_f, gi_f, odd, big_edit, wide_out, out)
    state = lambda: [(f.count(), raw(f), f.match_flags()[0].tobytes()) for f in folds]  # noqa: E731
    before = state()

    def refused(f, mode, o, code=_lib.E_ARG, unpaired=0):
        st = M.PairStats()
        rc = L.mtsv_fold_pair(f, mode, 100, unpaired, o, C.byref(st), None)
        assert rc == code, (rc, L.mtsv_last_error())
        assert state() == before
        return L.mtsv_last_error().decode()

    assert "odd" in refused(odd.h, M.PAIR_BOTH, out.h)                                   # an odd n_reads
    assert "MTSV_GRAIN_LONG" in refused(narrow_f.h, M.PAIR_PROPER, out.h)                # PROPER on a narrow grain
    assert "MTSV_GRAIN_LONG" in refused(gi_f.h, M.PAIR_PROPER, out.h)
    assert "itself" in refused(out.h, M.PAIR_BOTH, out.h)                                # out == f
    assert "MTSV_GRAIN_TAXID" in refused(even.h, M.PAIR_BOTH, wide_out.h)                # a wide out
    for mode in (-1, 3, 99):
        assert "mode" in refused(even.h, mode, out.h)                                   # a bad mode
    for mode in MODES.values():
        assert "2^31" in refused(big_edit.h, mode, out.h, unpaired=1)                    # edit >= 2^31, counted on the device
    assert "unpaired_edits" in refused(even.h, M.PAIR_EITHER, out.h, unpaired=2 ** 31)
    refused(None, M.PAIR_BOTH, out.h)
    refused(even.h, M.PAIR_BOTH, None)
    if M.device_count() > 1:
        far = M.Fold(1, M.GRAIN_TAXID, n_reads=4)
        refused(even.h, M.PAIR_BOTH, far.h)
        far.close()
    # and the calls they refused work
    for f, mode in ((even, R.PROPER), (narrow_f, R.BOTH), (gi_f, R.EITHER)):
        recs = PC.project(f.grain, [(0, 5, 1, 10, 1), (1, 5, 1, 20, 2)])
        assert check(f, recs, 6, mode, 100, 1, out=out) == [(0, 5, 3)]
    for f in folds:
        f.close()


# ---- 6. end to end ----

MAX_FRAGMENT, READ_LEN, EDIT_RATE = 500, 100, 0.13
# the mates' offsets are window starts: the match's start less up to the edit tolerance, cut at the bin's start
MAX_INSERT = MAX_FRAGMENT + int(READ_LEN * EDIT_RATE)
Pair = collections.namedtuple("Pair", "mates kind tax")


def cut_pairs(index_file, n_true=220, n_chimeric=30, n_lonely=30, n_mutated=20, seed=41):
    rng = random.Random(seed)
    bins = [b for b in index_file.bins if b[3] - b[2] > 2 * MAX_FRAGMENT]

    def fragment(b):
        while True:  # (the synthetic text holds runs of N, and a read of them has no hit in the reference either)
            length = rng.randrange(300, MAX_FRAGMENT + 1)
            start = rng.randrange(b[2], b[3] - length)
            frag = index_file.text[start:start + length]
            if b"N" not in frag[:READ_LEN] and b"N" not in frag[-READ_LEN:]:
                return frag

    def mates(frag):
        return [frag[:READ_LEN], helpers.revcomp(frag[-READ_LEN:])]

    pairs = []
    for k in range(n_true + n_mutated):
        b = rng.choice(bins)
        m = mates(fragment(b))
        if k >= n_true:
            j = rng.randrange(2)
            m[j] = helpers.mutate(rng, m[j], rng.randrange(1, 6), b"ACGT")
        pairs.append(Pair(m, "true" if k < n_true else "mutated", b[1]))
    for _ in range(n_chimeric):
        b0 = rng.choice(bins)
        b1 = rng.choice([b for b in bins if b[1] != b0[1]])
        pairs.append(Pair([mates(fragment(b0))[0], mates(fragment(b1))[1]], "chimeric", None))
    for _ in range(n_lonely):
        m = mates(fragment(rng.choice(bins)))
        m[rng.randrange(2)] = helpers.rnd_seq(rng, READ_LEN)
        pairs.append(Pair(m, "lonely", None))
    rng.shuffle(pairs)
    return pairs


def write_fastq(path, reads, ids):
    with open(path, "wb") as f:
        for r, i in zip(reads, ids):
            f.write(b"@" + i.encode() + b" some description\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_e2e")
    chunks = []
    for c, seed in enumerate((5, 6)):
        ix = M.MGIndex.synth(seed=seed, n_taxa=8, gis_per_taxon=2, seq_len=20000)
        p = str(d / f"chunk{c}.idx")
        ix.write(p)
        ix.to_device(0)
        chunks.append((ix, p))
    pairs = cut_pairs(pack_ref.IndexFile(chunks[0][1]))
    reads = [m for p in pairs for m in p.mates]
    # the mates share an ID, or a stem with /1 and /2
    pair_ids = [f"frag{k}" for k in range(len(pairs))]
    ids = [i + s for k, i in enumerate(pair_ids) for s in (("/1", "/2") if k % 2 else ("", ""))]
    fq = d / "interleaved.fastq"
    write_fastq(fq, reads, ids)
    # the library path: upload, run at LONG against every chunk, fold_add_run
    bases, off = helpers.reads_to_batch(reads)
    fold = M.Fold(0, M.GRAIN_LONG, n_reads=len(reads))
    for ix, _ in chunks:
        b = M.Batch(ix, 0, len(reads), len(bases), lanes=1)
        b.set_assignment_grain(M.GRAIN_LONG)
        b.set_assignments(M.ASSIGN_ONLY)
        b.upload(bases, off)
        b.run()
        fold.add_run(b)
        b.close()
    recs = [tuple(r) for r in fold.download_gi().tolist()]
    E = collections.namedtuple("E", "dir index fq pairs reads ids pair_ids fold recs chunk0")
    yield E(d, ",".join(p for _, p in chunks), fq, pairs, reads, ids, pair_ids, fold, recs, chunks[0][1])
    fold.close()


def holds_source_at_edit_0(pairs, joined):
    got = {(p, t): e for p, t, e in joined}
    return [k for k, p in enumerate(pairs) if p.kind == "true" and got.get((k, p.tax)) != 0]


def test_the_reference_alone_pairs_every_true_fragment(e2e):
    # the CPU oracle's hits through the restatement: the condition the library path is held to below is the reference's own
    from oracle import oracle as O
    bases, off = helpers.reads_to_batch(e2e.reads)
    hits, _ = O.Index.read(e2e.chunk0).bin_batch(bases, off, O.default_params(), threads=8)
    recs = [(int(h["read"]), int(h["tax_id"]), int(h["gi"]), int(h["offset"]), int(h["edit"])) for h in hits]
    assert holds_source_at_edit_0(e2e.pairs, R.pair(R.PROPER, recs, MAX_INSERT)) == []
    assert holds_source_at_edit_0(e2e.pairs, R.pair(R.PROPER, recs, 150)) != []         # ... and the window matters


@pytest.mark.parametrize("mode", list(MODES))
def test_library_path_on_binned_pairs(mode, e2e, monkeypatch):
    n_reads = len(e2e.reads)
    want = check(e2e.fold, e2e.recs, n_reads, MODES[mode], MAX_INSERT, 7, key=("e2e", "long"))
    assert len(want) > 200
    if mode == "proper":
        assert holds_source_at_edit_0(e2e.pairs, want) == []
        both = wanted(("e2e", "long"), R.BOTH, e2e.recs, MAX_INSERT, 7)
        assert set((p, t) for p, t, _ in want) <= set((p, t) for p, t, _ in both)       # the window and the GI only take away


def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


def pair_args(mode):
    return ["--fold-on-gpu", "--interleaved", "--pair-mode", mode, "--max-insert", MAX_INSERT] + (["--unpaired-penalty", 7] if mode == "either" else [])


VARIANTS = {
    "plain": [],
    "dedup_text_on_gpu": ["--dedup", "--text-on-gpu"],
    "blocks_that_end_on_a_mate_1": ["--batch-reads", "63", "--fold-reads", "190"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_binner_interleaved_writes_the_lines_of_the_restatement(mode, variant, e2e, tmp_path):
    want = wanted(("e2e", "long"), MODES[mode], e2e.recs, MAX_INSERT, 7)
    res, rep = tmp_path / "res.txt", tmp_path / "rep.tsv"
    r = run_binner("--fastq", e2e.fq, "-i", e2e.index, "-m", res, "--report", rep, *pair_args(mode), *VARIANTS[variant], env={"MTSV_CLI_TIMING": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert res.read_bytes() == R.lines(want, e2e.pair_ids) and len(want) > 200
    st = R.stats(e2e.recs, len(e2e.reads), want)
    line = re.search(r"Joined (\d+) pairs: both mates hit (\d+), one mate hit (\d+), joined (\d+)\.", r.stdout + r.stderr)
    assert line and [int(x) for x in line.groups()] == [st["pairs"], st["both_mates_hit"], st["one_mate_hit"], st["joined"]]
    assert re.search(r"\[cli pair timing\] pair device [\d.]+ ms", r.stderr)
    if variant == "blocks_that_end_on_a_mate_1":
        assert int(re.search(r"super_batches (\d+)", r.stderr).group(1)) > 2
    # the report counts pairs
    stats, total = F.report(want)
    rows = [l.split("\t") for l in rep.read_text().splitlines()[1:]]
    assert {int(x[0]): [int(x[1]), int(x[3]), int(x[5]), int(x[7])] for x in rows} == stats and total == st["joined"]


def test_binner_refuses_an_odd_number_of_records(e2e, tmp_path):
    fq, res = tmp_path / "odd.fastq", tmp_path / "res.txt"
    write_fastq(fq, e2e.reads[:41], e2e.ids[:41])
    r = run_binner("--fastq", fq, "-i", e2e.index, "-m", res, *pair_args("proper"), "--batch-reads", "8")
    assert r.returncode == 12, r.stdout + r.stderr
    assert re.search(r"Unable to read from input file: an interleaved input of an odd number of records: record 40 \('frag20'\) has no mate", r.stdout + r.stderr)


def test_binner_refuses_mates_whose_ids_do_not_agree(e2e, tmp_path):
    fq, res = tmp_path / "ids.fastq", tmp_path / "res.txt"
    ids = list(e2e.ids[:40])
    ids[22], ids[23] = "left/2", "left/1"                                               # pair 11: the stems agree, the mates are swapped
    write_fastq(fq, e2e.reads[:40], ids)
    r = run_binner("--fastq", fq, "-i", e2e.index, "-m", res, *pair_args("both"))
    assert r.returncode == 12, r.stdout + r.stderr
    assert re.search(r"Unable to read from input file: the mates of pair 11 of an interleaved input are named 'left/2' and 'left/1'", r.stdout + r.stderr)
