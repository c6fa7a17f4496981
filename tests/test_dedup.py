"""-m gpu tests of binning identical reads once (k_dedup.hip, mtsv_batch_take_unique, mtsv_fold_expand, mtsv-binner --dedup).

The grouping and the fan are compared with the plain-Python restatement (dedup_ref.py), record for record; the end-to-end and
command-line tests compare the path with dedup against the same path without it, byte for byte.  Every test runs with
MTSV_DEDUP_HASH_BITS unset, 3 (eight start slots, equal tags: long chains) and 0 (one chain, every compare runs in full); the
variable is read when a map is created, so a fresh map per test sees it."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import dedup_ref as D
import helpers
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib
from test_partition_cpu import write_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
BITS = [None, "3", "0"]
BITS_IDS = ["hash64", "hash3", "hash0"]
GRAINS = {"taxid": M.GRAIN_TAXID, "long": M.GRAIN_LONG, "taxid_gi": M.GRAIN_TAXID_GI}
N_LETTERS = b"NRYKMSWBDHVnx-*."


@pytest.fixture(scope="module")
def two_indexes(tmp_path_factory):
    d = tmp_path_factory.mktemp("dedup_idx")
    out = []
    for c, seed in enumerate((5, 6)):
        ix = M.MGIndex.synth(seed=seed, n_taxa=8, gis_per_taxon=2, seq_len=20000)
        p = str(d / f"chunk{c}.idx")
        ix.write(p)
        ix.to_device(0)
        out.append((ix, p))
    return out


@pytest.fixture(scope="module")
def ix(two_indexes):
    return two_indexes[0][0]


def set_bits(monkeypatch, bits):
    if bits is None:
        monkeypatch.delenv("MTSV_DEDUP_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("MTSV_DEDUP_HASH_BITS", bits)


# ---- 1. grouping ----

def variant(rng, r, kind):
    """a read that differs from r the way `kind` says; kinds 4 and 5 are duplicates of r once normalised"""
    b = bytearray(r)
    other = lambda c: rng.choice([x for x in b"ACGT" if x != (c & ~32)])  # noqa: E731
    if kind == 0 and b:
        b[0] = other(b[0])                                   # equal except the first base
    elif kind == 1 and b:
        b[-1] = other(b[-1])                                 # ... the last base
    elif kind == 2 and b:
        tail = (len(b) - 1) // 4 * 4                         # ... one base of the last (partial) dword
        i = rng.randrange(tail, len(b))
        b[i] = other(b[i])
    elif kind == 3:
        del b[-1:]                                           # a strict prefix
    elif kind == 4:
        b = bytearray(bytes(b).swapcase())                   # case only
    elif kind == 5:
        b = bytearray(rng.choice(N_LETTERS) if c not in b"ACGTacgt" else c for c in b)  # which letter stands for N
    return bytes(b)


def adversarial_reads(n, seed):
    """n reads of 0..300 bases at every byte alignment, about half of them copies or near-copies of earlier ones"""
    rng = random.Random(seed)
    reads = []
    for i in range(n):
        if reads and rng.random() < 0.5:
            src = reads[rng.randrange(len(reads))]
            reads.append(variant(rng, src, rng.randrange(8)))   # (6, 7: an exact copy)
        else:
            L = 0 if i % 97 == 50 else i % 300 + 1              # every residue modulo 4, and some empty reads
            reads.append(helpers.rnd_seq(rng, L, b"ACGTACGTACGTN"))
    if n > 1024:  # first occurrence the last read of the first 1024-read tile, its copy opens the next
        reads[1023] = helpers.rnd_seq(rng, 151)
        reads[1024] = reads[1023]
    return reads


def check_take(src, dst, m, raws, src_map=None):
    """take_unique(dst, src, m) on the batch `raws` that src holds, against the restatement; returns its representatives"""
    bases, off = helpers.reads_to_batch(raws)
    reads = D.read_codes(bases, off)
    want_read, want_rep = D.dupmap(reads, src_map)
    reps = D.representatives(reads)
    want_codes = b"".join(reads[j] for j in reps)
    n_unique, bases_kept, ms = dst.take_unique(src, m)
    assert (n_unique, bases_kept) == (len(reps), len(want_codes)) and ms >= 0.0
    read, rep, u = m.download()
    assert u == n_unique and read.dtype == np.uint64 and rep.dtype == np.uint64
    assert read.tolist() == want_read
    bad = np.nonzero(rep != np.array(want_rep, dtype=np.uint64))[0] if len(rep) == len(want_rep) else None
    assert bad is not None and len(bad) == 0, (len(rep), len(want_rep), None if bad is None else (bad[:10], rep[bad[:10]]))
    codes, roff = dst.download_reads()
    assert roff.tolist() == np.cumsum([0] + [len(reads[j]) for j in reps]).tolist()
    assert codes.tobytes() == want_codes
    assert dst.read_map().tolist() == [want_read[j] for j in reps]
    return reps


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
def test_grouping_equals_the_restatement_at_every_size(ix, bits, monkeypatch):
    """mtsv_batch_upload accepts reads of no bases: the read sets hold some, and they are each other's duplicates"""
    set_bits(monkeypatch, bits)
    cap_reads, cap_bases = 5100, 5100 * 160
    src, dst = M.Batch(ix, 0, cap_reads, cap_bases, lanes=1), M.Batch(ix, 0, cap_reads, cap_bases, lanes=1)
    m = M.DupMap(0)
    r0, p0, u0 = m.download()
    assert len(r0) == 0 and len(p0) == 0 and u0 == 0                    # before any take
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 5003):
        raws = adversarial_reads(n, 1000 + n)
        if n >= 1023:
            lens = {len(r) % 4 for r in raws}
            assert lens == {0, 1, 2, 3} and b"" in raws and max(map(len, raws)) >= 299
        bases, off = helpers.reads_to_batch(raws)
        src.upload(bases, off)
        reps = check_take(src, dst, m, raws)
        assert n == 1 or 1 < len(reps) < n, "the set must hold duplicates and distinct reads"
    # the same map and workspaces again: all identical (one slot, every group on the atomic min), then all distinct
    same = [helpers.rnd_seq(random.Random(3), 150)] * 3000
    src.upload(*helpers.reads_to_batch(same))
    assert check_take(src, dst, m, same) == [0]
    rng = random.Random(4)
    distinct = [helpers.rnd_seq(rng, 40 + i % 7) for i in range(3000)]
    src.upload(*helpers.reads_to_batch(distinct))
    assert len(check_take(src, dst, m, distinct)) == len(set(distinct))
    empty = [b""] * 70                                                  # nothing but reads of no bases
    src.upload(*helpers.reads_to_batch(empty))
    assert check_take(src, dst, m, empty) == [0]
    for b in (src, dst):
        b.close()
    m.close()


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
def test_named_pairs_are_told_apart_or_joined(ix, bits, monkeypatch):
    """the hand-written pairs of the issue, at every byte alignment of the second read of a pair"""
    set_bits(monkeypatch, bits)
    rng = random.Random(8)
    raws = []
    for L in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 149, 150, 151, 300):
        base = helpers.rnd_seq(rng, L, b"ACGTN" if L > 4 else b"ACGT")
        for kind in range(6):
            raws += [base, variant(rng, base, kind)]
        raws.append(b"A" * (len(raws) % 3 + 1))                         # moves the alignment of what follows
    bases, off = helpers.reads_to_batch(raws)
    reads = D.read_codes(bases, off)
    rep = D.rep(reads)
    # the pairs the restatement joins are exactly the kinds that collapse in the normalisation
    src, dst, m = M.Batch(ix, 0, len(raws), len(bases), lanes=1), M.Batch(ix, 0, len(raws), len(bases), lanes=1), M.DupMap(0)
    src.upload(bases, off)
    check_take(src, dst, m, raws)
    k = 0
    for L in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 149, 150, 151, 300):
        for kind in range(6):
            a, b = k + 2 * kind, k + 2 * kind + 1
            assert (reads[a] == reads[b]) == (kind >= 4), (L, kind)
            assert (rep[b] == rep[a]) == (kind >= 4)
        k += 13
    for b in (src, dst):
        b.close()
    m.close()


# ---- 2. a mapped source ----

def duplicated(rng, reads, share):
    """`share` of the reads replaced by copies of other reads of the list (of whatever kind those are)"""
    reads = list(reads)
    for i in rng.sample(range(len(reads)), int(share * len(reads))):
        reads[i] = reads[rng.randrange(len(reads))]
    return reads


def rows_of(bases, off):
    o = off.astype(np.int64)
    return [bytes(bases[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
def test_behind_take_reads_the_map_and_the_hits_carry_the_callers_numbers(two_indexes, bits, monkeypatch):
    set_bits(monkeypatch, bits)
    (ix_a, _), (ix_b, _) = two_indexes
    rng = random.Random(21)
    raws = rows_of(*M.synth_reads(ix_a, seed=3, n_reads=300, read_len=150)) + rows_of(*M.synth_reads(ix_b, seed=4, n_reads=400, read_len=150))
    rng.shuffle(raws)
    raws = duplicated(rng, raws, 0.4)
    bases, off = helpers.reads_to_batch(raws)
    n = len(raws)
    filt, mid, dst, full = (M.Batch(i, 0, n, len(bases), lanes=1) for i in (ix_a, ix_b, ix_b, ix_b))
    filt.set_match_flags(M.MATCH_ONLY)
    filt.upload(bases, off)
    filt.run()
    n_kept, _, _ = mid.take_reads(filt, M.KEEP_UNMATCHED)
    kept = mid.read_map()
    assert 0 < n_kept < n and len(kept) == n_kept
    m = M.DupMap(0)
    kept_raws = [raws[int(j)] for j in kept]
    reps = check_take(mid, dst, m, kept_raws, src_map=kept)              # read[] and rep[] are numbers of the 700
    assert len(reps) < n_kept
    rep_numbers = {int(kept[j]) for j in reps}
    dst.run()
    got = dst.download()
    full.upload(bases, off)
    full.run()
    want = full.download()
    want = want[np.isin(want["read"], np.array(sorted(rep_numbers), dtype=np.uint64))]
    assert len(want) > 0
    helpers.assert_same_hits(got, want)
    assert dst.stats()["n_reads"] == len(reps)
    for b in (filt, mid, dst, full):
        b.close()
    m.close()


# ---- 3. the fan ----

def seq_of(g):
    return bytes(b"ACGT"[(g >> (2 * k)) & 3] for k in range(12))


# (multiplicity, records of the representative)
FAN_GROUPS = [(500, 3000), (500, 1), (500, 0), (2, 3000), (2, 1), (2, 0), (1, 3000), (1, 1), (1, 0)]
_fan = {}


def fan_reads():
    rng = random.Random(77)
    raws = [seq_of(g) for g, (mult, _) in enumerate(FAN_GROUPS) for _ in range(mult)]
    rng.shuffle(raws)
    return raws


def records_for(grain, read, k):
    """k records of `read` in key order, TaxIDs on both sides of 2^31"""
    tax = lambda i: (10 + i) | ((i & 1) << 31)  # noqa: E731
    if grain == M.GRAIN_TAXID:
        return sorted((read, tax(i), (7 * i) % 23) for i in range(k))
    return sorted((read, tax(i // 3), i % 3, (5 * i) % 4099 if grain == M.GRAIN_LONG else 9 + i, (7 * i) % 23) for i in range(k))


def to_array(grain, recs):
    names = ("read", "tax_id", "edit") if grain == M.GRAIN_TAXID else ("read", "tax_id", "gi", "offset", "edit")
    out = np.zeros(len(recs), dtype=M.ASSIGN_DTYPE if grain == M.GRAIN_TAXID else M.ASSIGN_GI_DTYPE)
    cols = np.array(recs, dtype=np.uint64).reshape(-1, len(names))
    for k, f in enumerate(names):
        out[f] = cols[:, k]
    return out


def fan_case(grain):
    """(reads, records of the representatives, the restatement's expansion) -- computed once per grain, never changed"""
    if grain not in _fan:
        raws = fan_reads()
        reads = D.read_codes(*helpers.reads_to_batch(raws))
        read, rep = D.dupmap(reads)
        recs = []
        for j in D.representatives(reads):
            g = next(g for g in range(len(FAN_GROUPS)) if seq_of(g) == raws[j])
            recs += records_for(grain, j, FAN_GROUPS[g][1])
        want = D.expand(recs, read, rep)
        assert len(want) == sum(mu * k for mu, k in FAN_GROUPS) and len(recs) == sum(k for _, k in FAN_GROUPS)
        _fan[grain] = (raws, to_array(grain, recs), to_array(grain, want))
    return _fan[grain]


def download(fold):
    return fold.download() if fold.grain == M.GRAIN_TAXID else fold.download_gi()


def same_report_and_flags(a, b):
    ra, ta, _ = a.taxa_report()
    rb, tb, _ = b.taxa_report()
    assert ta == tb and len(ra) == len(rb) > 0
    for f in M.TAXON_STATS_DTYPE.names:                                   # (field by field: the rows carry padding)
        assert np.array_equal(ra[f], rb[f]), f
    fa, na = a.match_flags()
    fb, nb = b.match_flags()
    assert na == nb and np.array_equal(fa, fb) and 0 < na < len(fa)


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
@pytest.mark.parametrize("tile", ["64", None], ids=["tile64", "default_tile"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_fan_equals_the_restatement(ix, gname, tile, bits, monkeypatch, capfd):
    grain = GRAINS[gname]
    set_bits(monkeypatch, bits)
    monkeypatch.setenv("MTSV_TRACE", "1")
    if tile is None:
        monkeypatch.delenv("MTSV_FAN_TILE", raising=False)
    else:
        monkeypatch.setenv("MTSV_FAN_TILE", tile)
    raws, recs, want = fan_case(grain)
    bases, off = helpers.reads_to_batch(raws)
    n = len(raws)
    src, dst, m = M.Batch(ix, 0, n, len(bases), lanes=1), M.Batch(ix, 0, n, len(bases), lanes=1), M.DupMap(0)
    monkeypatch.delenv("MTSV_TRACE")
    src.upload(bases, off)
    assert dst.take_unique(src, m)[0] == len(FAN_GROUPS)
    f_rep, f_all, f_ref = M.Fold(0, grain, n), M.Fold(0, grain), M.Fold(0, grain, n)
    f_rep.add_records(recs)
    f_all.add_records(np.zeros(0, dtype=recs.dtype))
    assert f_all.expand(f_rep, m) >= 0.0
    err = capfd.readouterr().err
    assert re.search(r"\[dedup\] %d of %d reads distinct" % (len(FAN_GROUPS), n), err)
    assert re.search(r"\[expand\] %d records of .* -> %d records of %d reads in tiles of %s:" % (len(recs), len(want), n, tile or "1024"), err), err
    got = download(f_all)
    assert f_all.count() == len(want) and got.tobytes() == want.tobytes()
    assert download(f_rep).tobytes() == recs.tobytes()                   # the source is not changed
    f_ref.add_records(want)
    same_report_and_flags(f_all, f_ref)
    # (the first expansion grew the fold) a second one goes into the other array of the fold that now holds records
    assert f_all.expand(f_rep, m) >= 0.0 and download(f_all).tobytes() == want.tobytes()
    for x in (src, dst, f_rep, f_all, f_ref, m):
        x.close()


def test_fan_into_a_fold_that_holds_records_grows_it_then_reuses_it(ix, monkeypatch):
    """The three ways an expansion finds room in a destination that already holds records, each compared byte for byte with
    the restatement: a new pair of arrays (one held record gave the fold room for 65 536; 33 000 sequences twice with one
    record per representative expand to 66 000), the fold's other array (the same expansion again), and the other array
    again for a result of four records."""
    set_bits(monkeypatch, None)
    grain, n_seq = M.GRAIN_TAXID, 33000
    seqs = [bytes(b"ACGT"[(g >> (2 * k)) & 3] for k in range(20)) for g in range(n_seq)]
    raws = seqs + seqs
    random.Random(78).shuffle(raws)
    bases, off = helpers.reads_to_batch(raws)
    n = len(raws)
    reads = D.read_codes(bases, off)
    read, rep = D.dupmap(reads)
    reps = D.representatives(reads)
    recs = [(j, (10 + j % 7) | ((j & 1) << 31), j % 23) for j in reps]
    two = recs[:1] + recs[-1:]
    want, want_two = D.expand(recs, read, rep), D.expand(two, read, rep)
    assert len(reps) == n_seq and len(want) == n > 65536 and len(want_two) == 4
    src, dst, m = M.Batch(ix, 0, n, len(bases), lanes=1), M.Batch(ix, 0, n, len(bases), lanes=1), M.DupMap(0)
    src.upload(bases, off)
    assert dst.take_unique(src, m)[0] == n_seq
    held = np.array([(n - 1, 4, 4)], dtype=M.ASSIGN_DTYPE)
    f_rep, f_two, f_dst = M.Fold(0, grain, n), M.Fold(0, grain, n), M.Fold(0, grain, n)
    f_rep.add_records(to_array(grain, recs))
    f_two.add_records(to_array(grain, two))
    f_dst.add_records(held)
    for source, expected in ((f_rep, want), (f_rep, want), (f_two, want_two)):
        assert f_dst.expand(source, m) >= 0.0
        assert f_dst.count() == len(expected) and f_dst.download().tobytes() == to_array(grain, expected).tobytes()
    assert f_rep.download().tobytes() == to_array(grain, recs).tobytes()   # the source is not changed
    # the fold goes on as any other: the next list is folded out of the array the last expansion wrote
    f_dst.add_records(held)
    assert f_dst.download().tobytes() == to_array(grain, sorted(want_two + [(n - 1, 4, 4)])).tobytes()
    for x in (src, dst, m, f_rep, f_two, f_dst):
        x.close()


def test_fan_groups_are_what_they_claim():
    raws = fan_reads()
    reads = D.read_codes(*helpers.reads_to_batch(raws))
    mult = {}
    for k in D.rep(reads):
        mult[k] = mult.get(k, 0) + 1
    assert sorted(mult.values()) == sorted(mu for mu, _ in FAN_GROUPS) and len(set(raws)) == len(FAN_GROUPS)


# ---- 4. refusals ----

@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
def test_refusals_leave_the_destination_and_the_map_as_they_were(ix, bits, monkeypatch):
    set_bits(monkeypatch, bits)
    raws = [b"ACGTACGTAC", b"TTTTACGTAC", b"ACGTACGTAC", b"GGGTACGTAC", b"TTTTACGTAC", b"ACGTACGTAC"]   # rep 0 1 0 3 1 0
    bases, off = helpers.reads_to_batch(raws)
    n = len(raws)
    src, dst, small = M.Batch(ix, 0, n, len(bases), lanes=1), M.Batch(ix, 0, n, len(bases), lanes=1), M.Batch(ix, 0, 2, len(bases), lanes=1)
    m, fresh = M.DupMap(0), M.DupMap(0)
    src.upload(bases, off)
    check_take(src, dst, m, raws)
    before = [x.tolist() for x in m.download()[:2]]
    assert before == [[0, 1, 2, 3, 4, 5], [0, 1, 0, 3, 1, 0]]

    def refused(call, *args):
        with pytest.raises(M.MtsvError) as e:
            call(*args)
        assert e.value.code == _lib.E_ARG, str(e.value)

    # a take that does not fit: three representatives, a destination for two; the destination keeps its own batch
    keep = [b"GATTACA", b"CAT"]
    small.upload(*helpers.reads_to_batch(keep))
    refused(small.take_unique, src, m)
    codes, roff = small.download_reads()
    assert codes.tobytes() == b"".join(D.read_codes(*helpers.reads_to_batch(keep))) and roff.tolist() == [0, 7, 10]
    assert [x.tolist() for x in m.download()[:2]] == before
    refused(dst.take_unique, dst, m)                                     # into itself
    nothing = M.Batch(ix, 0, n, len(bases), lanes=1)
    refused(dst.take_unique, nothing, m)                                 # nothing resident in the source
    assert [x.tolist() for x in m.download()[:2]] == before and dst.read_map().tolist() == [0, 1, 3]
    # the fan
    good = np.array([(0, 7, 1), (0, 9, 2), (3, 7, 0)], dtype=M.ASSIGN_DTYPE)
    stray = np.array([(0, 7, 1), (2, 7, 1)], dtype=M.ASSIGN_DTYPE)        # read 2 is a copy of read 0
    held = np.array([(5, 4, 4)], dtype=M.ASSIGN_DTYPE)
    f_src, f_stray, f_dst, f_wide = M.Fold(0, M.GRAIN_TAXID, n), M.Fold(0, M.GRAIN_TAXID, n), M.Fold(0, M.GRAIN_TAXID, n), M.Fold(0, M.GRAIN_LONG, n)
    f_src.add_records(good)
    f_stray.add_records(stray)
    f_dst.add_records(held)
    refused(f_dst.expand, f_stray, m)                                    # a record of a read that represents nothing
    refused(f_dst.expand, f_dst, m)                                      # into itself
    refused(f_wide.expand, f_src, m)                                     # another grain
    refused(f_dst.expand, f_src, fresh)                                  # a map without a take
    assert f_dst.download().tobytes() == held.tobytes() and f_dst.count() == 1 and f_wide.count() == 0
    assert f_dst.expand(f_src, m) >= 0.0
    want = D.expand([tuple(int(v) for v in r) for r in good.tolist()], *before)
    assert [tuple(r) for r in f_dst.download().tolist()] == want and len(want) == 7
    for x in (src, dst, small, nothing, m, fresh, f_src, f_stray, f_dst, f_wide):
        x.close()


# ---- 5. end to end ----

@pytest.fixture(scope="module")
def e2e_reads(ix):
    rng = random.Random(31)
    raws = rows_of(*M.synth_reads(ix, seed=12, n_reads=4000, read_len=150))
    for i in range(len(raws)):
        x = rng.random()
        if x < 0.30:
            raws[i] = helpers.mutate(rng, raws[i], rng.randrange(1, 30))
        elif x < 0.42:
            raws[i] = helpers.rnd_seq(rng, rng.randrange(30, 200))        # no hit
    return duplicated(rng, raws, 0.4)


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
@pytest.mark.parametrize("gname", list(GRAINS))
def test_dedup_path_gives_the_fold_of_the_plain_path(ix, e2e_reads, gname, bits, monkeypatch):
    grain = GRAINS[gname]
    set_bits(monkeypatch, bits)
    raws = e2e_reads
    bases, off = helpers.reads_to_batch(raws)
    n = len(raws)
    reads = D.read_codes(bases, off)
    reps = D.representatives(reads)
    assert 0.55 * n < len(reps) < 0.8 * n
    ids = [f"r{i}/x" for i in range(n)]

    def workspace():
        b = M.Batch(ix, 0, n, len(bases), lanes=1)
        b.set_assignment_grain(grain)
        b.set_assignments(M.ASSIGN_ONLY)
        return b

    # A: upload, run, fold
    a, f_a = workspace(), M.Fold(0, grain, n)
    a.upload(bases, off)
    a.run()
    f_a.add_run(a)
    # B: upload, take_unique, run, fold, expand
    intake, b, m = M.Batch(ix, 0, n, len(bases), lanes=1), workspace(), M.DupMap(0)
    f_rep, f_b = M.Fold(0, grain, n), M.Fold(0, grain)
    intake.upload(bases, off)
    n_unique, _, _ = b.take_unique(intake, m)
    assert n_unique == len(reps)
    b.run()
    assert b.stats()["n_reads"] == n_unique
    f_rep.add_run(b)
    f_b.expand(f_rep, m)
    got, want = download(f_b), download(f_a)
    assert len(want) > n // 2 and f_rep.count() < f_a.count()
    assert got.tobytes() == want.tobytes()
    unmatched_copies = set(range(n)) - set(reps) - set(want["read"].tolist())
    assert unmatched_copies, "copies of reads that get no hit"
    assert f_b.format_text(ids)[0] == f_a.format_text(ids)[0]
    same_report_and_flags(f_b, f_a)
    for x in (a, intake, b, m, f_a, f_rep, f_b):
        x.close()


# ---- 6. the command line ----

@pytest.fixture(scope="module")
def cli(two_indexes, tmp_path_factory):
    (ix_a, pa), (ix_b, pb) = two_indexes
    d = tmp_path_factory.mktemp("dedup_cli")
    rng = random.Random(41)
    raws = rows_of(*M.synth_reads(ix_a, seed=13, n_reads=200, read_len=150)) + rows_of(*M.synth_reads(ix_b, seed=14, n_reads=200, read_len=150))
    raws += [helpers.rnd_seq(rng, 150) for _ in range(60)]
    rng.shuffle(raws)
    raws = duplicated(rng, raws, 0.4)
    raws = [r.lower() if i % 11 == 0 else r for i, r in enumerate(raws)]      # a copy in another case is still a copy
    recs = [(b"read%d" % i, b"", r, bytes(rng.choice(b"FGHIJ") for _ in r)) for i, r in enumerate(raws)]
    fq = d / "reads.fastq"
    write_input(fq, recs, [r[0] for r in recs], True, False)
    return f"{pa},{pb}", fq, raws, d, {}


def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


CLI_CASES = {
    "default": [],
    "long": ["--output-format", "long"],
    "text_on_gpu": ["--text-on-gpu"],
    "long_text_on_gpu": ["--output-format", "long", "--text-on-gpu"],
    "pieces_of_64": ["--batch-reads", "64", "--fold-reads", "200"],
}


@pytest.mark.parametrize("bits", BITS, ids=BITS_IDS)
@pytest.mark.parametrize("case", list(CLI_CASES))
def test_binner_dedup_writes_the_same_files(cli, case, bits, tmp_path):
    index, fq, raws, shared, plain_done = cli
    env = {"MTSV_CLI_TIMING": "1"}
    if bits is not None:
        env["MTSV_DEDUP_HASH_BITS"] = bits
    names = ("res.txt", "rep.tsv", "u.fq")
    got = [tmp_path / ("dedup_" + x) for x in names]
    ref = [shared / (f"plain_{case}_" + x) for x in names]   # the run without the switch: once per case, then only read
    for extra, (res, rep, u) in ((["--dedup"], got), ([], ref)):
        if not extra and case in plain_done:
            continue
        r = run_binner("--fastq", fq, "-i", index, "-m", res, "--fold-on-gpu", "--report", rep, "--unmatched", u, *CLI_CASES[case], *extra, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        line = re.search(r"Collapsed (\d+) reads to (\d+) distinct sequences\.", r.stdout)
        timing = re.search(r"\[cli dedup timing\] take_unique device ([\d.]+) ms, expand device ([\d.]+) ms", r.stderr)
        assert re.search(r"\[cli fold timing\] super_batches \d+ chunks 2 reads %d;" % len(raws), r.stderr)
        if not extra:
            assert line is None and timing is None
            plain_done[case] = True
            continue
        assert timing
        reads = D.read_codes(*helpers.reads_to_batch(raws))
        n_distinct = len(D.representatives(reads))
        assert int(line.group(1)) == len(raws)
        if case == "pieces_of_64":   # (a sequence is counted once per piece that holds it)
            assert n_distinct <= int(line.group(2)) < len(raws)
        else:
            assert int(line.group(2)) == n_distinct and n_distinct < 0.8 * len(raws)
    for a, b in zip(got, ref):
        assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 0
    assert 0 < got[2].read_bytes().count(b"\n+\n") < len(raws) and got[0].read_bytes().count(b"\n") > 200
