"""-m gpu tests of chaining workspaces (k_compact.hip, mtsv_batch_take_reads / _read_map / _download_reads, mtsv-binner
--filter-index): the unmatched (matched) reads of one run become the resident batch of another workspace on the device, and
the second run's hits carry the caller's read numbers.

What a compaction must produce is the numpy restatement (chain_ref.py) applied to the normalised input; expected hits and
flags come from the CPU oracle, never from the device's own hits.  Only the first group takes the device's match flags as
its INPUT (the flags themselves are test_match_flags.py's subject): 100 003 reads are too many for the oracle here."""
import os
import random
import subprocess

import numpy as np
import pytest

import chain_ref as CR
import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_partition_cpu import golden_records, write_input
from test_taxa_report import PARAM_SETS, both_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
KEEPS = {"unmatched": M.KEEP_UNMATCHED, "matched": M.KEEP_MATCHED}
N_SYNTH = 100_003          # many scan tiles, not a multiple of 64, three lanes on the host path (>= 98304)


def presence(hits, n):
    p = np.zeros(n, dtype=bool)
    p[hits["read"].astype(np.int64)] = True
    return p


def both_kinds(p):
    assert 0 < int(p.sum()) < len(p), "the fixture must hold matched and unmatched reads"
    return p


def check_compaction(dst, taken, bases, off, mask, src_map=None, what=""):
    """dst after take_reads (which returned `taken`) against the restatement on the reads mask keeps; returns the map"""
    want_codes, want_off, want_map = CR.compact(CR.normalise(bases), off, mask, src_map)
    n_kept, bases_kept, ms = taken
    assert (n_kept, bases_kept) == (len(want_map), len(want_codes)), what
    assert ms >= 0.0
    codes, roff = dst.download_reads()
    rmap = dst.read_map()
    assert roff.dtype == np.uint64 and rmap.dtype == np.uint64 and codes.dtype == np.uint8
    assert np.array_equal(roff, want_off), what
    assert np.array_equal(rmap, want_map), what
    bad = np.nonzero(codes != want_codes)[0] if len(codes) == len(want_codes) else None
    assert bad is not None and len(bad) == 0, (what, len(codes), len(want_codes), None if bad is None else bad[:10])
    return rmap


# ---- the kernels against numpy on many tiles, with the device's flags as input ----

@pytest.fixture(scope="module")
def synth():
    ix = M.MGIndex.synth(seed=5, n_taxa=24, gis_per_taxon=2, seq_len=20000)
    ix.to_device(0)
    bases, off = M.synth_reads(ix, seed=9, n_reads=N_SYNTH, read_len=150)
    return ix, bases, off


@pytest.mark.parametrize("fill", ["upload_run", "run_host_one_lane", "run_host_three_lanes"])
def test_compaction_of_100003_reads_equals_the_restatement(synth, fill):
    ix, bases, off = synth
    src = M.Batch(ix, 0, N_SYNTH, len(bases), lanes=1 if fill == "run_host_one_lane" else 0)
    src.set_match_flags(M.MATCH_ONLY)
    if fill == "upload_run":
        src.upload(bases, off)
        src.run()
    else:
        src.run_host(bases, off)
        assert src.stats()["n_lanes"] == (1 if fill == "run_host_one_lane" else 3)
    flags, n_matched = src.match_flags()
    both_kinds(flags)
    assert 0.05 < 1.0 - n_matched / N_SYNTH < 0.2            # about 10 % unmatched (the random reads of mtsv_synth_reads)
    dst = M.Batch(ix, 0, N_SYNTH, len(bases))
    for kname, keep in KEEPS.items():
        taken = dst.take_reads(src, keep)
        check_compaction(dst, taken, bases, off, CR.keep_mask(flags, keep == M.KEEP_MATCHED), what=(fill, kname))
        dst.run()
        assert dst.stats()["n_reads"] == taken[0]
    dst.close()
    src.close()


# ---- ragged lengths: every residue of source and destination offsets, the two edges of a read, a read of many trips ----

LENGTHS = (0, 1, 3, 17, 18, 63, 64, 65, 150, 151, 320)
LONG = 5000


@pytest.fixture(scope="module")
def tricky(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.to_device(0)
    return ix, O.Index.read(p), entries, gene, unit


@pytest.fixture(scope="module")
def ragged(tricky):
    """reads whose lengths cycle through LENGTHS, cut from tricky_reads (hits, as a rule) and from random sequence (none) in
    an irregular order, one read of LONG bases among them; the oracle says which of them have a hit"""
    ix, orc, entries, gene, unit = tricky
    rng = random.Random(77)
    pool = [r for r in helpers.tricky_reads(entries, gene, unit, seed=13, n_each=30, lengths=(150, 320)) if len(r) >= 64]
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    reads = []
    for k in range(14 * len(LENGTHS)):
        L = LENGTHS[k % len(LENGTHS)]
        if rng.random() < 0.45:
            reads.append(helpers.rnd_seq(rng, L))
        else:
            r = rng.choice([q for q in pool if len(q) >= L] or pool)
            if L <= 18:                                      # short enough to need an exact piece of the database for a hit
                t = rng.choice(texts)
                st = rng.randrange(0, len(t) - 20)
                r = t[st:st + L]
            reads.append(r[:L])
        assert len(reads[-1]) == L
    reads.insert(37, helpers.rnd_seq(rng, LONG))             # kept by KEEP_UNMATCHED: 79 trips of a 16-lane group
    reads.insert(90, max(texts, key=len))                    # a whole database sequence: a long read with a hit
    bases, off = helpers.reads_to_batch(reads)
    lens = np.diff(off.astype(np.int64))
    assert {int(x) % 4 for x in off[:-1]} == {0, 1, 2, 3} and len({int(x) % 16 for x in off[:-1]}) == 16
    want, _ = orc.bin_batch(bases, off, O.default_params(), threads=8)
    flags = both_kinds(presence(want, len(reads)))
    # kept and dropped reads of every length class: the copy meets each length on both sides
    for L in LENGTHS[5:]:
        assert flags[lens == L].any() and not flags[lens == L].all(), L
    assert not flags[37] and flags[90] and lens[90] > 2000
    assert (flags[1:] != flags[:-1]).sum() > len(reads) // 4   # kept and dropped reads alternate irregularly
    return ix, reads, flags


def sub_batch(reads, idx):
    return helpers.reads_to_batch([reads[i] for i in idx])


def ragged_cases(reads, flags):
    n = len(reads)
    hit, miss = np.nonzero(flags)[0], np.nonzero(~flags)[0]
    return {
        "all_reads": list(range(n)),
        "one_read_matched": [int(hit[0])],
        "one_read_unmatched": [int(miss[0])],
        "only_matched": hit.tolist(),
        "only_unmatched": miss.tolist(),
        "63_reads": list(range(63)),
        "64_reads": list(range(64)),
        "65_reads": list(range(65)),
        "ends_on_the_long_read": list(range(38)),
        "starts_with_the_long_read": list(range(37, 137)),
    }


@pytest.mark.parametrize("case", ["all_reads", "one_read_matched", "one_read_unmatched", "only_matched", "only_unmatched", "63_reads", "64_reads",
                                  "65_reads", "ends_on_the_long_read", "starts_with_the_long_read"])
def test_ragged_reads_both_keeps(ragged, case):
    ix, reads, flags = ragged
    idx = ragged_cases(reads, flags)[case]
    bases, off = sub_batch(reads, idx)
    f = flags[idx]
    src = M.Batch(ix, 0, len(idx), max(len(bases), 1))
    src.set_match_flags(M.MATCH_ONLY)
    src.upload(bases, off)
    src.run()
    got_flags, _ = src.match_flags()
    assert np.array_equal(got_flags, f)
    dst = M.Batch(ix, 0, len(idx), max(len(bases), 1))
    for kname, keep in KEEPS.items():
        mask = CR.keep_mask(f, keep == M.KEEP_MATCHED)
        taken = dst.take_reads(src, keep)
        check_compaction(dst, taken, bases, off, mask, what=(case, kname))
        dst.run()
        st, hits = dst.stats(), dst.download()
        assert st["n_reads"] == int(mask.sum())
        if keep == M.KEEP_UNMATCHED or not mask.any():       # the same index: what it did not match has no hit (m = 0: an empty run)
            assert len(hits) == 0 and st["n_hits"] == 0
        else:
            assert np.array_equal(np.unique(hits["read"]), np.nonzero(mask)[0])   # every kept read hits again, under its own number
    dst.close()
    src.close()


# ---- end to end: a filter index and a database that share sequences, against the oracle ----

class Pair:
    """the oracle's view of a chain: per parameter set, the flags of every stage's index over ALL reads (reads are binned
    independently, so a stage's flags over its survivors are a subset of these) and the database's hits over any subset"""

    def __init__(self, filters, db, bases, off):
        self.filters, self.db, self.bases, self.off = filters, db, bases, off
        self.n = len(off) - 1
        self._flags, self._hits = {}, {}

    def flags(self, pname, k):
        if (pname, k) not in self._flags:
            _, op = both_params(**PARAM_SETS[pname])
            want, _ = self.filters[k].bin_batch(self.bases, self.off, op, threads=8)
            self._flags[pname, k] = presence(want, self.n)
        return self._flags[pname, k]

    def db_hits(self, pname, survivors):
        """the oracle on the database over reads `survivors` (ascending indices), read = the original number"""
        key = (pname, tuple(survivors.tolist()))
        if key not in self._hits:
            _, op = both_params(**PARAM_SETS[pname])
            sb, so = sub_batch_arrays(self.bases, self.off, survivors)
            want, _ = self.db.bin_batch(sb, so, op, threads=8)
            local = want["read"].astype(np.int64)
            want = want.copy()
            want["read"] = survivors[local]
            self._hits[key] = (want, presence_local(local, len(survivors)))
        return self._hits[key]


def presence_local(local, n):
    p = np.zeros(n, dtype=bool)
    p[local] = True
    return p


def sub_batch_arrays(bases, off, idx):
    o = off.astype(np.int64)
    parts = [bases[o[i]:o[i + 1]] for i in idx]
    out = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    so = np.zeros(len(idx) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=so[1:])
    return out, so


@pytest.fixture(scope="module")
def chain(tricky, tmp_path_factory):
    """D = the tricky database; F = every third sequence of it plus unrelated random sequences, also cut into the chunk list
    F1 (the shared sequences) and F2 (the unrelated ones plus two more shared).  Reads from D (150 and 320 bases, the tiled
    path), from F's own sequences, and random ones."""
    ix_d, orc_d, entries, gene, unit = tricky
    rng = random.Random(2024)
    shared = entries[::3]
    own = [(700000 + k, 90000 + k, helpers.rnd_seq(rng, 2500)) for k in range(6)]
    d = tmp_path_factory.mktemp("filter")
    made = {}
    for name, ent in (("F", shared + own), ("F1", shared[:-2]), ("F2", own + shared[-2:])):
        ix = M.MGIndex.build(ent, threads=4)
        p = str(d / f"{name}.idx")
        ix.write(p)
        ix.to_device(0)
        made[name] = (ix, O.Index.read(p))
    reads = helpers.tricky_reads(entries, gene, unit, seed=31, n_each=24, lengths=(150, 320))
    for k in range(70):                                      # F only
        t = own[k % len(own)][2]
        L = 320 if k % 7 == 0 else 150
        st = rng.randrange(0, len(t) - L)
        r = helpers.mutate(rng, t[st:st + L], rng.randrange(0, 12))
        reads.append(r if k % 2 else helpers.revcomp(r))
    reads += [helpers.rnd_seq(rng, rng.choice((150, 151, 320))) for _ in range(50)]   # neither
    rng.shuffle(reads)
    assert max(map(len, reads)) > 256 and len(reads) < 3000
    bases, off = helpers.reads_to_batch(reads)
    one = Pair([made["F"][1]], orc_d, bases, off)
    two = Pair([made["F1"][1], made["F2"][1]], orc_d, bases, off)
    return ix_d, made, bases, off, one, two


def run_chain(stages, ix_d, bases, off, mp, vmode, n, report=True):
    """upload + run on the first filter, take_reads down the chain; returns (filter workspaces, database workspace)"""
    fws = []
    for ix in stages:
        b = M.Batch(ix, 0, n, len(bases))
        b.set_verify_mode(vmode)
        b.set_match_flags(M.MATCH_ONLY)
        fws.append(b)
    dst = M.Batch(ix_d, 0, n, len(bases))
    dst.set_verify_mode(vmode)
    dst.set_match_flags(M.MATCH_WITH_HITS)
    if report:
        dst.set_taxa_report(True)
    fws[0].upload(bases, off)
    fws[0].run(mp)
    for k in range(1, len(fws)):
        fws[k].take_reads(fws[k - 1], M.KEEP_UNMATCHED)
        fws[k].run(mp)
    taken = dst.take_reads(fws[-1])                          # (the default: KEEP_UNMATCHED)
    dst.run(mp)
    return fws, dst, taken


@pytest.mark.parametrize("vmode", [0, 1], ids=["reference_order", "edit_first"])
@pytest.mark.parametrize("pname", ["default", "stress", "one_assignment"])
def test_filter_then_database_equals_the_oracle(chain, pname, vmode):
    ix_d, made, bases, off, one, _ = chain
    n = one.n
    mp, _ = both_params(**PARAM_SETS[pname])
    in_f = one.flags(pname, 0)
    survivors = np.nonzero(~in_f)[0]
    want, hit_d = one.db_hits(pname, survivors)
    # the oracle sees all four classes: in F only, in D only, in both, in neither
    all_d, _ = one.db_hits(pname, np.arange(n))
    in_d = presence(all_d, n)
    for cls in (in_f & ~in_d, ~in_f & in_d, in_f & in_d, ~in_f & ~in_d):
        assert cls.any()
    fws, dst, taken = run_chain([made["F"][0]], ix_d, bases, off, mp, vmode, n)
    check_compaction(dst, taken, bases, off, ~in_f, what=pname)
    got = dst.download()
    assert len(want) > 0
    assert_same_hits(got, want)
    assert np.all(np.diff(got["read"].astype(np.int64)) >= 0)
    st = dst.stats()
    assert st["n_reads"] == len(survivors) and st["n_hits"] == len(want)
    # the database workspace's own flags and report are per resident read; the map translates
    flags, n_matched = dst.match_flags()
    assert np.array_equal(flags, hit_d) and n_matched == int(hit_d.sum())
    assert np.array_equal(np.unique(got["read"]), dst.read_map()[flags])
    rows, total, _ = dst.taxa_report()
    assert total == int(hit_d.sum()) and len(rows) > 0
    dst.close()
    fws[0].close()


def test_two_filter_stages_compose_their_maps(chain):
    ix_d, made, bases, off, _, two = chain
    n = two.n
    mp, _ = both_params()
    f1, f2 = two.flags("default", 0), two.flags("default", 1)
    assert (f1 & ~f2).any() and (~f1 & f2).any() and (~f1 & ~f2).any()
    survivors = np.nonzero(~f1 & ~f2)[0]
    want, _ = two.db_hits("default", survivors)
    fws, dst, taken = run_chain([made["F1"][0], made["F2"][0]], ix_d, bases, off, mp, 0, n, report=False)
    # stage by stage: F2's workspace holds what F1 left, under F1's numbering
    s1 = np.nonzero(~f1)[0]
    assert np.array_equal(fws[1].read_map(), s1.astype(np.uint64))
    flags2, _ = fws[1].match_flags()
    assert np.array_equal(flags2, f2[s1])
    own = np.nonzero(~f2[s1])[0]                             # the second step's own map: positions among F1's survivors
    assert np.array_equal(dst.read_map(), CR.compose(s1, own)) and np.array_equal(dst.read_map(), survivors.astype(np.uint64))
    check_compaction(dst, taken, bases, off, ~f1 & ~f2, what="two stages")
    assert len(want) > 0
    assert_same_hits(dst.download(), want)
    # a matched-side chain on the same workspaces: the reads F1 leaves and F2 matches
    taken = dst.take_reads(fws[1], M.KEEP_MATCHED)
    check_compaction(dst, taken, bases, off, ~f1 & f2, what="unmatched by F1, matched by F2")
    dst.run(mp)
    want_m, _ = two.db_hits("default", np.nonzero(~f1 & f2)[0])
    assert_same_hits(dst.download(), want_m)
    for b in fws + [dst]:
        b.close()


# ---- state ----

def test_upload_drops_the_map_and_take_reads_repeats(chain):
    ix_d, made, bases, off, one, _ = chain
    n = one.n
    mp, _ = both_params()
    in_f = one.flags("default", 0)
    survivors = np.nonzero(~in_f)[0]
    want, _ = one.db_hits("default", survivors)
    all_d, _ = one.db_hits("default", np.arange(n))
    fws, dst, taken = run_chain([made["F"][0]], ix_d, bases, off, mp, 0, n, report=False)
    assert_same_hits(dst.download(), want)
    # the same hand-over again, into the same destination
    again = dst.take_reads(fws[0], M.KEEP_UNMATCHED)
    assert again[:2] == taken[:2]
    check_compaction(dst, again, bases, off, ~in_f)
    dst.run(mp)
    assert_same_hits(dst.download(), want)
    dst.run(mp)                                              # and a second run of the same resident codes
    assert_same_hits(dst.download(), want)
    # upload on the compacted workspace: a plain run again, numbered by itself
    dst.upload(bases, off)
    assert np.array_equal(dst.read_map(), np.arange(n, dtype=np.uint64))
    codes, roff = dst.download_reads()
    assert np.array_equal(codes, CR.normalise(bases)) and np.array_equal(roff, off)
    dst.run(mp)
    assert_same_hits(dst.download(), all_d)
    assert np.array_equal(dst.read_map(), np.arange(n, dtype=np.uint64))
    # ... and a host batch on a compacted workspace is numbered by itself too
    dst.take_reads(fws[0])
    dst.run_host(bases, off, mp)
    assert_same_hits(dst.download(), all_d)
    dst.close()
    fws[0].close()


def test_what_take_reads_refuses(chain, monkeypatch):
    ix_d, made, bases, off, one, _ = chain
    n = one.n
    in_f = one.flags("default", 0)
    src = M.Batch(made["F"][0], 0, n, len(bases))
    dst = M.Batch(ix_d, 0, n, len(bases))

    def refused(d, s, keep=M.KEEP_UNMATCHED, says=None):
        with pytest.raises(M.MtsvError) as e:
            d.take_reads(s, keep)
        assert e.value.code == _lib.E_ARG, str(e.value)
        assert says is None or says in str(e.value), str(e.value)

    src.upload(bases, off)
    src.run()
    refused(dst, src, says="match flags")                    # flags off
    src.set_match_flags(M.MATCH_WITH_HITS)
    refused(dst, src, says="no completed run")               # flags on, but no run since
    src.upload(bases, off)
    refused(dst, src, says="no completed run")               # uploaded, not run
    src.run()
    refused(src, src, says="itself")
    refused(dst, src, keep=2, says="keep")
    refused(dst, src, keep=-1, says="keep")
    small_reads = M.Batch(ix_d, 0, int((~in_f).sum()) - 1, len(bases))
    refused(small_reads, src, says="survive")
    small_bases = M.Batch(ix_d, 0, n, 1000)
    refused(small_bases, src, says="survive")
    for b in (small_reads, small_bases):                      # as they were: nothing resident, an empty identity map
        assert len(b.read_map()) == 0
        b.close()
    # the same source and destination still work
    check_compaction(dst, dst.take_reads(src), bases, off, ~in_f)
    check_compaction(dst, dst.take_reads(src, M.KEEP_MATCHED), bases, off, in_f)
    # a host batch that took turns through two input segments has lost its first reads
    bases3 = np.tile(bases, 3)
    off3 = np.concatenate([off[:-1] + np.uint64(k * len(bases)) for k in range(3)] + [np.array([3 * len(bases)], dtype=np.uint64)])
    src3 = M.Batch(made["F"][0], 0, 3 * n, len(bases3))
    src3.set_match_flags(M.MATCH_ONLY)
    dst3 = M.Batch(ix_d, 0, 3 * n, len(bases3))
    monkeypatch.setenv("MTSV_ARENA_BASES", "65536")
    assert len(bases3) > 2 * 65536
    src3.run_host(bases3, off3)
    monkeypatch.delenv("MTSV_ARENA_BASES")
    flags, _ = src3.match_flags()
    assert np.array_equal(flags, np.tile(in_f, 3))
    refused(dst3, src3, says="no longer in HBM")
    src3.run_host(bases3, off3)                              # one segment: fine
    check_compaction(dst3, dst3.take_reads(src3), bases3, off3, ~np.tile(in_f, 3))
    src3.close()
    dst3.close()
    src.run_host(bases, off)
    with pytest.raises(M.MtsvError) as e:                    # the source's own resident batch was a host batch: nothing to show
        src.download_reads()
    assert e.value.code == _lib.E_ARG
    dst.close()
    src.close()


# ---- mtsv-binner --filter-index ----

def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """the golden database D, a filter F built from its first records, the golden reads as FASTQ and FASTA, and the result
    lines the oracle derives: oracle on F, then on D over the survivors"""
    d = tmp_path_factory.mktemp("cli")
    db_fasta = os.path.join(GOLD, "e2e_db.fasta")
    lines = open(db_fasta).read().splitlines(keepends=True)
    starts = [i for i, l in enumerate(lines) if l.startswith(">")]
    f_fasta = d / "filter.fasta"
    f_fasta.write_text("".join(lines[:starts[12]]))          # the first twelve records
    idx_d, idx_f = str(d / "D.idx"), str(d / "F.idx")
    M.MGIndex.build_fasta(db_fasta, threads=4).write(idx_d)
    M.MGIndex.build_fasta(str(f_fasta), threads=4).write(idx_f)
    forms = {}
    for name, fastq in (("fastq", True), ("fasta", False)):
        recs, headers = golden_records(fastq)
        path = d / f"reads.{name}"
        write_input(path, recs, headers, fastq, False)
        forms[name] = (path, fastq, recs)
    reads = [r[2] for r in forms["fastq"][2]]
    ids = [r[0].decode() for r in forms["fastq"][2]]
    bases, off = helpers.reads_to_batch(reads)
    pair = Pair([O.Index.read(idx_f)], O.Index.read(idx_d), bases, off)
    in_f = both_kinds(pair.flags("default", 0))
    want, hit_d = pair.db_hits("default", np.nonzero(~in_f)[0])
    assert hit_d.any() and len(want) > 0
    want_lines = {long_fmt: sorted(M.format_results(want, ids, long_format=long_fmt).splitlines()) for long_fmt in (False, True)}
    return idx_d, idx_f, forms, in_f, want, want_lines


@pytest.mark.parametrize("extra", [("--devices", "0"), ("--devices", "0,0", "--batch-reads", "9")], ids=["one_worker", "two_workers_small_batches"])
@pytest.mark.parametrize("form", ["fastq", "fasta"])
def test_cli_filter_index_equals_the_oracle_and_the_two_step_run(cli, tmp_path, form, extra):
    idx_d, idx_f, forms, in_f, want, want_lines = cli
    path, fastq, recs = forms[form]
    kind = "--fastq" if fastq else "--fasta"
    res = tmp_path / "res.txt"
    r = run_binner(kind, path, "-i", idx_d, "-m", res, "--filter-index", idx_f, *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    got = sorted(res.read_text().splitlines())
    assert got == want_lines[False] and len(got) > 0
    assert f"removed {int(in_f.sum())} of {len(in_f)} reads" in r.stdout
    # the two-step run through a file
    tmp, res2 = tmp_path / ("tmp.fq" if fastq else "tmp.fa"), tmp_path / "res2.txt"
    assert run_binner(kind, path, "-i", idx_f, "--unmatched", tmp, *extra).returncode == 0
    assert run_binner(kind, tmp, "-i", idx_d, "-m", res2, *extra).returncode == 0
    assert sorted(res2.read_text().splitlines()) == got
    # the long format and the report, once each
    if form == "fastq":
        long_res = tmp_path / "long.txt"
        r = run_binner(kind, path, "-i", idx_d, "-m", long_res, "--filter-index", idx_f, "--output-format", "long", *extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(long_res.read_text().splitlines()) == want_lines[True]
    else:
        import taxa_report_ref as R
        rep, res3 = tmp_path / "report.tsv", tmp_path / "res3.txt"
        r = run_binner(kind, path, "-i", idx_d, "-m", res3, "--filter-index", idx_f, "--report", rep, *extra, env={"MTSV_CLI_CLEAN_EXIT": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(res3.read_text().splitlines()) == got
        stats, total = R.classify_hits(want)
        assert rep.read_bytes() == M.format_taxa_report(R.rows_array(stats, M.TAXON_STATS_DTYPE), total)


def test_cli_filter_chain_of_two_and_read_offset(cli, tmp_path):
    idx_d, idx_f, forms, in_f, want, want_lines = cli
    path, fastq, recs = forms["fastq"]
    # the same filter twice: the second stage removes nothing, the results are the same
    res = tmp_path / "res.txt"
    r = run_binner("--fastq", path, "-i", idx_d, "-m", res, "--filter-index", f"{idx_f},{idx_f}", "--batch-reads", "50")
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(res.read_text().splitlines()) == want_lines[False]
    assert f"Filter stage 2 ({idx_f}): removed 0 of {int((~in_f).sum())} reads" in r.stdout
    # --read-offset 100: the reads from 100 on, filtered and binned
    ids = [rec[0].decode() for rec in recs]
    keep = {i for i in ids[100:]}
    off_res = tmp_path / "off.txt"
    r = run_binner("--fastq", path, "-i", idx_d, "-m", off_res, "--filter-index", idx_f, "--read-offset", "100")
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(off_res.read_text().splitlines()) == [l for l in want_lines[False] if l.rsplit(":", 1)[0] in keep]
    # a missing filter index is the usual error
    r = run_binner("--fastq", path, "-i", idx_d, "-m", tmp_path / "x.txt", "--filter-index", tmp_path / "missing.idx")
    assert r.returncode == 2 and "Error running query" in r.stdout
