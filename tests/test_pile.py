"""-m gpu tests of the pileup (k_pile.hip, mtsv_pileup, mtsv-binner --variants).

Crafted hits go in through mtsv_pileup_add_run(hits != NULL), so the kernels are tested without binning; real runs pile the
hits where they lie on the device.  Expected values never come from the device: they are pile_ref's, which walks place_ref's
edit scripts base by base.  Every comparison is exact: the download of every reference, slot by slot, and the sites.
MTSV_PILE_TILE is read when an accumulator is created."""
import os
import random
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import pile_cases as PL
import pile_ref as PR
import place_cases as PC
import place_ref as R
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
STRESS = dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5)
ALL = PR.SLACK_ALL


def workspace(ix, reads, **kw):
    bases, off = helpers.reads_to_batch(reads)
    b = M.Batch(ix, 0, max(len(reads), 1), max(len(bases), 1), **kw)
    b.upload(bases, off)
    return b


def site_tuples(rows):
    return [(int(r["tax_id"]), int(r["gi"]), int(r["pos"]), int(r["ref"]), r["n"].tolist()) for r in rows]


def same(p, table, seq, *thresholds):
    """every reference of the accumulator against pile_ref's table, and the sites under (0, 0, 0) and the thresholds given"""
    assert p.info()["n_refs"] == len(table) and p.info()["n_slots"] == sum(len(s) for s in table.values())
    for key, slots in table.items():
        counts, codes = p.download(*key)
        assert counts.shape == (len(slots), 8) and codes.tolist() == PR.ref_codes(seq[key]), key
        bad = np.nonzero((counts != np.array(slots, dtype=np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, (key, int(bad[0]), counts[bad[0]].tolist(), slots[bad[0]])
    for th in ((0, 0, 0),) + thresholds:
        assert site_tuples(p.sites(*th)[0]) == PR.sites(table, seq, *th), th


def state(p, keys):
    return p.info(), [(c.tobytes(), r.tobytes()) for c, r in (p.download(*k) for k in keys)]


@pytest.fixture(scope="module")
def crafted():
    entries = PC.database()
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    reads, hits = PC.crafted(entries)
    hits = PL.with_more_hits(reads, hits)
    place = PL.Placer(entries, PL.second_chunk())
    return ix, entries, reads, hits, place


def expected(entries, reads, hits, place, slack, taxa=None, table=None):
    table = PR.new_table(entries, taxa) if table is None else table
    return table, PR.add_run(table, reads, hits, place(reads, hits), slack)


# ---- 1. crafted hits, under both tiles ----

@pytest.mark.parametrize("tile", ["64", None], ids=["tile_64", "tile_default"])
def test_crafted_hits(crafted, tile, monkeypatch):
    ix, entries, reads, hits, place = crafted
    if tile:
        monkeypatch.setenv("MTSV_PILE_TILE", tile)
    assert len(hits) >= 250 and {len(r) for r in reads} >= {1, 256} and {h[5] for h in hits} == {0, 1}
    table, (piled, skipped) = expected(entries, reads, hits, place, ALL)
    b, p = workspace(ix, reads), M.Pileup(0)
    got = p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)
    assert got[:2] == (piled, skipped) == (len(hits), 0) and got[2] > 0
    same(p, table, PL.seq_of(entries), (1, 1, 0), (2, 2, 500000))
    assert p.info()["n_segments"] == 1 and p.info()["hits_piled"] == piled and p.info()["device_bytes"] >= 33 * 4 * (PC.BIN_LEN + 1)
    p.close()
    b.close()


# ---- 2. batch sizes ----

@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_batch_sizes(crafted, n):
    ix, entries, reads, hits, place = crafted
    sub = [hits[(7 * k) % len(hits)] for k in range(n)]                        # any order, hits repeated
    b, p = workspace(ix, reads), M.Pileup(0)
    got = p.add_run(b, PC.hits_array(sub, M.HIT_DTYPE), 1)
    if n == 0:                                                                 # nothing is launched, no reference is learnt
        assert got == (0, 0, 0.0) and p.info() == dict(n_refs=0, n_slots=0, n_segments=0, device_bytes=0, hits_piled=0, hits_skipped=0)
        assert len(p.sites()[0]) == 0
    else:
        table, (piled, skipped) = expected(entries, reads, sub, place, 1)
        assert got[:2] == (piled, skipped) and got[2] > 0
        same(p, table, PL.seq_of(entries))
    p.close()
    b.close()


# ---- 3. the deep pile ----

def test_the_deep_pile(crafted):
    ix, entries, _, _, place = crafted
    reads, hits, planted = PL.deep_pile(entries)
    table, (piled, skipped) = expected(entries, reads, hits, place, 0)
    b, p = workspace(ix, reads), M.Pileup(0)
    assert p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), 0)[:2] == (1000, 0) == (piled, skipped)
    counts, _ = p.download(*PL.DEEP_KEY)
    snp, dele, ins = counts[planted["snp"]], counts[planted["del"]], counts[planted["ins"]]
    assert int(snp[:7].sum()) == 1000 and int(snp[1 + planted["snp_base"]]) == 300 and int(dele[6]) == 100 and int(ins[7]) == 50
    site = (PL.DEEP_KEY[0], PL.DEEP_KEY[1], planted["snp"])
    at = lambda *th: {s[:3] for s in site_tuples(p.sites(*th)[0])}
    assert site in at(0, 0, 300000) and site not in at(0, 0, 300001) and site not in at(0, 301, 0) and site in at(1000, 300, 0)
    assert at(1001, 0, 0) == set()
    same(p, table, PL.seq_of(entries), (0, 0, 300000), (0, 0, 300001), (0, 301, 0), (1001, 0, 0), (1000, 50, 50000))
    p.close()
    b.close()


# ---- 4. slack ----

@pytest.mark.parametrize("slack", [0, 1, 2, ALL])
def test_slack_on_reads_with_several_hits(crafted, slack):
    ix, entries, reads, hits, place = crafted
    table, (piled, skipped) = expected(entries, reads, hits, place, slack)
    assert piled == len(hits) - {0: 24, 1: 12}.get(slack, 0)
    b, p = workspace(ix, reads), M.Pileup(0)
    assert p.add_run(b, PC.hits_array(hits[::-1], M.HIT_DTYPE), slack)[:2] == (piled, 0)
    same(p, table, PL.seq_of(entries))
    p.close()
    b.close()


# ---- 5. the TaxID list ----

def test_a_taxa_list_skips_the_other_references(crafted):
    ix, entries, reads, hits, place = crafted
    table, (piled, skipped) = expected(entries, reads, hits, place, 0, taxa={2})
    whole, _ = expected(entries, reads, hits, place, 0)
    b, p = workspace(ix, reads), M.Pileup(0, taxa=[2, 2, 77])
    assert p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), 0)[:2] == (piled, skipped) and skipped == sum(h[1] != 2 for h in hits) > 0
    assert p.info()["n_refs"] == 2 and p.info()["hits_skipped"] == skipped and sorted(table) == [(2, 20), (2, 21)]
    same(p, table, PL.seq_of(entries))
    assert all(table[k] == whole[k] for k in table)                            # ... equal to the unfiltered run's
    with pytest.raises(M.MtsvError) as e:
        p.download(1, 10)
    assert e.value.code == _lib.E_ARG and "holds no reference (tax_id 1, gi 10)" in str(e.value)
    p.close()
    b.close()


# ---- 6. two chunks, one accumulator ----

def test_two_chunks_and_a_chunk_loaded_again(crafted):
    ix_a, entries_a, reads_a, hits_a, place = crafted
    entries_b = PL.second_chunk()
    reads_b, hits_b = PC.crafted(entries_b, seed=19)
    hits_b = hits_b[::3]
    ix_b = M.MGIndex.build(entries_b, threads=4)
    ix_b.to_device(0)
    seq = PL.seq_of(entries_a, entries_b)
    p = M.Pileup(0)
    table = {}
    for ix, entries, reads, hits in ((ix_b, entries_b, reads_b, hits_b), (ix_a, entries_a, reads_a, hits_a)):   # the later segment holds the smaller keys
        table.update(PR.new_table(entries))
        expected(entries, reads, hits, place, ALL, table=table)
        b = workspace(ix, reads)
        p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)
        b.close()
    assert p.info()["n_segments"] == 2 and p.info()["n_refs"] == 8
    same(p, table, seq, (1, 1, 0))
    again = M.MGIndex.build(entries_b, threads=4)                               # the first chunk as a new handle
    again.to_device(0)
    b = workspace(again, reads_b)
    p.add_run(b, PC.hits_array(hits_b, M.HIT_DTYPE), ALL)
    expected(entries_b, reads_b, hits_b, place, ALL, table=table)
    assert p.info()["n_segments"] == 2 and p.info()["n_refs"] == 8
    same(p, table, seq)
    single, _ = expected(entries_b, reads_b, hits_b, place, ALL)
    assert all(table[k] == [[2 * x for x in n] for n in single[k]] for k in single)     # that reference's counters double
    for w in (b, p, again, ix_b):
        w.close()


# ---- 7. slot L ----

def test_the_slot_l_read(crafted):
    ix, entries, _, _, place = crafted
    read, hit = PL.slot_l_read(entries)
    table, _ = expected(entries, [read], [hit], place, 0)
    assert table[PL.SLOT_L_KEY][PC.BIN_LEN][7] == 1
    b, p = workspace(ix, [read]), M.Pileup(0)
    assert p.add_run(b, PC.hits_array([hit], M.HIT_DTYPE))[:2] == (1, 0)
    same(p, table, PL.seq_of(entries))
    last = p.sites()[0][-1]
    assert (int(last["pos"]), int(last["ref"]), last["n"].tolist()) == (PC.BIN_LEN, M.PILE_REF_NONE, [0, 0, 0, 0, 0, 0, 0, 1])
    p.close()
    b.close()


# ---- 8. a real run, the hits where they lie ----

def test_the_hits_of_a_run_where_they_lie():
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=24)
    place, seq, want = PL.Placer(entries), PL.seq_of(entries), None
    for mode in (M.ASSIGN_OFF, M.ASSIGN_ONLY):
        b = workspace(ix, reads)
        b.set_assignments(mode)
        b.run(M.default_params(**STRESS))
        if mode == M.ASSIGN_OFF:
            down = b.download()
            assert len(down) > 10
            hits = [tuple(int(h[k]) for k in ("read", "tax_id", "gi", "offset", "edit", "strand")) for h in down]
            want = expected(entries, reads, hits, place, 0)
        else:
            assert len(b.download()) == 0                                       # the hits stay on the device
        table, (piled, skipped) = want
        p = M.Pileup(0)
        got = p.add_run(b)
        assert got[:2] == (piled, skipped) and 0 < piled <= len(hits) and got[2] > 0
        same(p, table, seq, (1, 1, 0))
        p.close()
        b.close()
    ix.close()


# ---- 9. refusals ----

def refused(p, b, hits, code, *words):
    with pytest.raises(M.MtsvError) as e:
        p.add_run(b, hits, ALL)
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_accumulator_as_it_was(crafted, monkeypatch):
    ix, entries, reads, hits, place = crafted
    seq = PL.seq_of(entries)
    good = PC.hits_array(hits, M.HIT_DTYPE)
    keys = sorted(seq)
    b, p = workspace(ix, reads), M.Pileup(0)
    table, _ = expected(entries, reads, hits, place, ALL)
    p.add_run(b, good, ALL)
    before = state(p, keys)

    def one_bad(k, **field):
        h = good.copy()
        for name, v in field.items():
            h[name][k] = v
        return h

    k = max(range(len(hits)), key=lambda i: hits[i][4])                        # the heaviest script
    r, t, g, o, e, strand = hits[k]
    m = R.min_edit(R.strand_codes(reads[r], strand), R.codes(seq[(t, g)][o:]))
    cases = [
        (one_bad(k, edit=m - 1), _lib.E_ARG, ("1 of %d hits are unplaceable" % len(hits), f"the first is hit {k} ")),
        (one_bad(5, gi=999), _lib.E_ARG, ("1 name a (tax_id, gi) the index does not hold", "the first is hit 5 ")),
        (one_bad(9, offset=PC.BIN_LEN), _lib.E_ARG, ("1 lie at or beyond the end of their bin",)),
        (one_bad(3, read=len(reads)), _lib.E_ARG, ("1 name a read that is not resident",)),
        (one_bad(70, strand=2), _lib.E_ARG, ("1 carry a strand above 1", "the first is hit 70 ")),
        (None, _lib.E_ARG, ("no completed run",)),
    ]
    for h, code, words in cases:
        refused(p, b, h, code, *words)
        assert state(p, keys) == before
    long_b = workspace(ix, reads[:3] + [helpers.rnd_seq(random.Random(1), 257)])
    refused(p, long_b, good[:1], _lib.E_LIMIT, "a read of 257 bases")
    long_b.close()
    host_b = M.Batch(ix, 0, 16, 4096)
    refused(p, host_b, good[:1], _lib.E_ARG, "holds no resident batch")
    host_b.run_host(*helpers.reads_to_batch(reads[:4]))
    refused(p, host_b, None, _lib.E_ARG, "host batch")
    host_b.close()
    assert state(p, keys) == before
    # a (tax_id, gi) the accumulator holds, with another length
    short = M.MGIndex.build([(1, 10, entries[0][2][:3000])] + entries[1:], threads=2)
    short.to_device(0)
    short_b = workspace(short, reads)
    at = next(i for i, h in enumerate(hits) if h[1] == 2)
    refused(p, short_b, good[at:at + 1], _lib.E_ARG, "reference (tax_id 1, gi 10) has 3000 bases in this index and 4200 in the pileup")
    assert state(p, keys) == before
    # a segment the device has no room for: of a second chunk, and of a fresh accumulator
    entries_b = PL.second_chunk()
    reads_b, hits_b = PC.crafted(entries_b, seed=19)
    ix_b = M.MGIndex.build(entries_b, threads=4)
    ix_b.to_device(0)
    b_b, good_b = workspace(ix_b, reads_b), PC.hits_array(hits_b[:40], M.HIT_DTYPE)
    fresh = M.Pileup(0)
    monkeypatch.setenv("MTSV_ALLOC_REFUSE", "the pileup segment")
    refused(p, b_b, good_b, _lib.E_NOMEM, "no memory for the pileup segment")
    refused(fresh, b, good, _lib.E_NOMEM, "no memory for the pileup segment")
    monkeypatch.delenv("MTSV_ALLOC_REFUSE")
    assert state(p, keys) == before and p.info()["n_segments"] == 1
    assert fresh.info() == dict(n_refs=0, n_slots=0, n_segments=0, device_bytes=0, hits_piled=0, hits_skipped=0)
    # the next valid call is what it is on a fresh accumulator
    p.add_run(b, good, ALL)
    expected(entries, reads, hits, place, ALL, table=table)
    same(p, table, seq)
    fresh.add_run(b, good, ALL)
    single, _ = expected(entries, reads, hits, place, ALL)
    same(fresh, single, seq)
    for w in (fresh, p, b_b, ix_b, short_b, short, b):
        w.close()


# ---- 10. reset ----

def test_reset_keeps_the_references(crafted):
    ix, entries, reads, hits, place = crafted
    seq, keys = PL.seq_of(entries), sorted(PL.seq_of(entries))
    good = PC.hits_array(hits, M.HIT_DTYPE)
    b, p = workspace(ix, reads), M.Pileup(0)
    p.add_run(b, good, 0)
    first = state(p, keys)
    p.reset()
    info = p.info()
    assert (info["n_refs"], info["n_segments"], info["hits_piled"], info["hits_skipped"]) == (4, 1, 0, 0) and info["device_bytes"] == first[0]["device_bytes"]
    same(p, PR.new_table(entries), seq)
    assert len(p.sites()[0]) == 0
    p.add_run(b, good, 0)
    assert state(p, keys) == first and p.info()["n_segments"] == 1
    p.close()
    b.close()


# ---- 11. mtsv-binner --fold-on-gpu --variants ----

@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("pile_e2e")
    chunks = [PC.database(seed=5, first_tax=1), PL.second_chunk()]
    reads, ids, (snp_key, snp_pos) = PL.snp_reads(chunks)
    fq = d / "reads.fastq"
    with open(fq, "wb") as f:
        for r, i in zip(reads, ids):
            f.write(b"@" + i.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bases, off = helpers.reads_to_batch(reads)
    paths, runs = [], []
    for c, entries in enumerate(chunks):
        ix = M.MGIndex.build(entries, threads=4)
        paths.append(str(d / f"chunk{c}.idx"))
        ix.write(paths[-1])
        ix.to_device(0)
        b = M.Batch(ix, 0, len(reads), len(bases), lanes=1)
        b.upload(bases, off)
        b.run()
        runs.append([tuple(int(h[k]) for k in ("read", "tax_id", "gi", "offset", "edit", "strand")) for h in b.download()])
        b.close()
        ix.close()
    place = PL.Placer(*chunks)

    def want(taxa, *th):
        table = {}
        for entries, hits in zip(chunks, runs):                                 # a call per chunk: the best edit is the chunk's
            table.update(PR.new_table(entries, taxa))
            PR.add_run(table, reads, hits, place(reads, hits), 0)
        return table, PR.sites(table, PL.seq_of(*chunks), *th)

    return d, ",".join(paths), fq, want, snp_key + (snp_pos,)


def binner(tmp_path, name, index, fq, *extra):
    res = tmp_path / f"{name}.res"
    r = subprocess.run([BINNER, *map(str, ["--fastq", fq, "-i", index, "-m", res, "--fold-on-gpu", "--batch-reads", "16", *extra])], capture_output=True,
                       text=True, timeout=600, env={**os.environ, "MTSV_CLI_TIMING": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    return res.read_bytes(), r.stderr


def test_binner_variants_are_the_restatements_text(e2e, tmp_path):
    d, index, fq, want, site = e2e
    var, aln, aln2 = tmp_path / "var.tsv", tmp_path / "aln.tsv", tmp_path / "aln2.tsv"
    plain, err = binner(tmp_path, "plain", index, fq)
    assert len(plain) > 0 and "[cli variants timing]" not in err
    with_var, err = binner(tmp_path, "var", index, fq, "--variants", var)
    table, rows = want(None, 1, 1, 0)
    assert with_var == plain and var.read_text() == PR.text(rows)
    assert "[cli variants timing] hits piled " in err and "sites %d;" % len(rows) in err
    n = table[site[:2]][site[2]]
    assert site in {r[:3] for r in rows} and PR.depth(n) >= 8 and max(n[1:5]) >= 6 and n[0] >= 2      # the planted SNP, and reads without it
    binner(tmp_path, "aln", index, fq, "--alignments", aln)
    ppm = max(n[1:5]) * 1000000 // PR.depth(n)
    for at, listed in ((ppm, True), (ppm + 1, False)):
        res, _ = binner(tmp_path, "both%d" % at, index, fq, "--alignments", aln2, "--variants", var, "--variant-taxa", "2,11", "--min-alt-frac", "%.6f" % (at / 1e6),
                        "--min-depth", "2", "--min-alt-reads", "2")
        _, rows = want({2, 11}, 2, 2, at)
        assert res == plain and var.read_text() == PR.text(rows) and (site in {r[:3] for r in rows}) == listed
        assert aln2.read_bytes() == aln.read_bytes() and len(aln.read_bytes()) > 0
