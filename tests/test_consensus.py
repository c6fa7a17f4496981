"""-m gpu tests of the consensus (k_cons.hip, mtsv_pileup_consensus, mtsv_pileup_add_counts, mtsv-binner --consensus).

Expected values never come from the device: they are cons_ref's, over pile_ref's table.  Every comparison is exact: every row
and every byte of the text.  Count tables go in through mtsv_pileup_add_counts, so ties and thresholds are reached directly.
MTSV_PILE_TILE is read when an accumulator is created."""
import os
import subprocess

import numpy as np
import pytest

import cons_cases as CC
import cons_ref as CR
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
BUILD = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-build")
ALL = PR.SLACK_ALL
DEFAULT = (1, 500000, 0, 0, 60)


def workspace(ix, reads):
    bases, off = helpers.reads_to_batch(reads)
    b = M.Batch(ix, 0, max(len(reads), 1), max(len(bases), 1))
    b.upload(bases, off)
    return b


def row_tuples(rows):
    return [tuple(int(r[f]) for f in CR.FIELDS) for r in rows]


def same(p, table, seq, *params):
    """the text and the rows under every parameter set against cons_ref's, and the rows again without the text"""
    for ps in params or (DEFAULT,):
        want_text, want_rows = CR.consensus(table, seq, *ps)
        text, rows, ms = p.consensus(*ps)
        assert row_tuples(rows) == want_rows, ps
        assert text.decode() == want_text, ps
        none, rows_only, _ = p.consensus(*ps, fasta=False)
        assert none is None and row_tuples(rows_only) == want_rows, ps
        assert M.format_consensus_stats(rows) == CR.stats_text(want_rows)


def state(p, keys):
    return p.info(), [(c.tobytes(), r.tobytes()) for c, r in (p.download(*k) for k in keys)]


def add_table(p, tables, n_hits=CC.ADD_HITS):
    for key, slots in tables.items():
        p.add_counts(key[0], key[1], 0, np.array(slots, dtype=np.uint32), n_hits)


@pytest.fixture(scope="module")
def crafted():
    entries = PC.database()
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    reads, hits = PC.crafted(entries)
    hits = PL.with_more_hits(reads, hits)
    st = CC.strain(entries)
    n = len(reads)
    reads = reads + st["reads"]
    hits = hits + [(h[0] + n,) + tuple(h[1:]) for h in st["hits"]]
    place = PL.Placer(entries, PL.second_chunk())
    table = PR.new_table(entries)
    PR.add_run(table, reads, hits, place(reads, hits), ALL)
    return ix, entries, reads, hits, place, table, st


@pytest.fixture(scope="module")
def small():
    entries = CC.small_database()
    ix = M.MGIndex.build(entries, threads=2)
    ix.to_device(0)
    reads, hits = CC.small_read(entries)
    table = PR.new_table(entries)
    PR.add_run(table, reads, hits, PL.Placer(entries)(reads, hits), 0)
    return ix, entries, reads, hits, table


def small_pileup(small):
    ix, entries, reads, hits, table = small
    b, p = workspace(ix, reads), M.Pileup(0)
    assert p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), 0)[:2] == (1, 0)
    b.close()
    assert p.info()["n_refs"] == len(CC.SMALL_REFS) and p.info()["n_slots"] == sum(L + 1 for _, _, L in CC.SMALL_REFS)
    return p, {k: [list(n) for n in v] for k, v in table.items()}


# ---- 1. crafted hits and the strain, under both tiles ----

@pytest.mark.parametrize("write", ["plain", "staged"])
@pytest.mark.parametrize("tile", ["64", None], ids=["tile_64", "tile_default"])
def test_crafted_hits_and_the_strain(crafted, tile, write, monkeypatch):
    ix, entries, reads, hits, place, table, st = crafted
    monkeypatch.setenv("MTSV_CONS_WRITE", write)                               # (read when an accumulator is created, as the tile is)
    if tile:
        monkeypatch.setenv("MTSV_PILE_TILE", tile)
    seq = PL.seq_of(entries)
    b, p = workspace(ix, reads), M.Pileup(0)
    assert p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)[:2] == (len(hits), 0)
    same(p, table, seq, DEFAULT, (CC.STRAIN_DEPTH, 500000, 0, 1, 60), (2, 900000, 100000, 0, 0), (0, 0, 0, 1, 1), (1, 1000000, 400000, 1, 4200))
    text, rows, ms = p.consensus(CC.STRAIN_DEPTH, 500000, 0, 0, 0)
    assert ms > 0 and st["expected"] in text.decode().split(">%d-%d\n" % (st["key"][1], st["key"][0]))[1].split("\n")[0]
    p.close()
    b.close()


# ---- 2. references that meet at chosen lanes, through add_counts ----

@pytest.mark.parametrize("write", ["plain", "staged"])
@pytest.mark.parametrize("tile", ["64", "128", None], ids=["tile_64", "tile_128", "tile_default"])
def test_count_tables_on_references_that_meet_at_tile_edges(small, tile, write, monkeypatch):
    monkeypatch.setenv("MTSV_CONS_WRITE", write)
    if tile:
        monkeypatch.setenv("MTSV_PILE_TILE", tile)
    ix, entries, *_ = small
    seq = PL.seq_of(entries)
    p, table = small_pileup(small)
    more = CC.random_tables(entries)
    add_table(p, more)
    CC.add_tables(table, more)
    assert p.info()["hits_piled"] == 1 + CC.ADD_HITS * len(more)
    for key, slots in table.items():                                           # download after add equals the sum
        counts, _ = p.download(*key)
        assert counts.tolist() == slots, key
    same(p, table, seq, DEFAULT, (2, 500000, 0, 1, 7), (0, 0, 0, 0, 0), (3, 750000, 250000, 1, 1), (1, 1000000, 0, 0, 64))
    text = p.consensus(*DEFAULT)[0].decode()
    assert ">30-3\n>31-3\n" in text                                            # deleted at every position: the header line alone
    p.close()


# ---- 3. ties, thresholds, line widths, fills, breadth ----

@pytest.mark.parametrize("write", ["plain", "staged"])
def test_ties_thresholds_widths_fills_and_breadth(small, write, monkeypatch):
    monkeypatch.setenv("MTSV_CONS_WRITE", write)
    ix, entries, *_ = small
    seq = PL.seq_of(entries)
    p, table = small_pileup(small)
    edge = {(1, 10): CC.edge_table(62), (1, 11): CC.edge_table(63, 0), (2, 21): CC.edge_table(128, 1)}
    full = {(2, 20): [[0, 0, 0, 0, 0, 0, 0, 0] if k >= 16 else [2, 0, 0, 0, 0, 0, 0, 0] for k in range(65)],   # breadth 16 / 64
            (3, 31): [[5, 0, 0, 0, 0, 0, 0, 0]] * 298 + [[0, 0, 0, 0, 0, 0, 5, 0], [0] * 8]}                 # cons_len 298
    for more in (edge, full):
        add_table(p, more)
        CC.add_tables(table, more)
    params = [(md, ppm, 0, fill, 60) for md in (0, 1, 2, 3, 4) for ppm in (0, 500000, 500001, 1000000) for fill in (0, 1)]
    params += [(1, 500000, 0, 0, w) for w in (0, 1, 298, 297, 299, 149, 62, 31)]                              # cons_len = w, w + 1, w - 1, 2 w
    params += [(1, 500000, b, 1, 60) for b in (250000, 250001, 1000000)]                                       # (2, 20) exactly at its breadth
    same(p, table, seq, *params)
    at, above = (row_tuples(p.consensus(1, 500000, b, 0, 60, fasta=False)[1]) for b in (250000, 250001))
    assert (2, 20) in {r[:2] for r in at} and (2, 20) not in {r[:2] for r in above}
    rows = {r[:2]: dict(zip(CR.FIELDS, r)) for r in row_tuples(p.consensus(2, 500000, 0, 0, 60)[1])}
    assert rows[(1, 10)]["ins_sites"] == 4 and rows[(1, 11)]["ins_sites"] == 3                                 # slot L of (1, 10) is one
    p.close()


# ---- 4. chunks whose keys interleave across segments ----

def test_segments_interleave_by_key(crafted):
    ix_a, entries_a, reads_a, hits_a, _, _, _ = crafted
    entries_b = PL.second_chunk()                                              # TaxIDs 10 .. 12, piled first: the later segment holds the smaller keys
    entries_c = [(2, 25, entries_b[0][2]), (5, 1, entries_b[1][2])]            # ... and these lie between and behind the first chunk's
    seq = PL.seq_of(entries_a, entries_b, entries_c)
    place = PL.Placer(entries_a, entries_b, entries_c)
    p, table = M.Pileup(0), {}
    for entries in (entries_b, entries_c, entries_a):
        if entries is entries_a:
            ix, reads, hits = ix_a, reads_a, hits_a
        else:
            ix = M.MGIndex.build(entries, threads=2)
            ix.to_device(0)
            reads, hits = PC.crafted((entries + entries_b)[:4], seed=19)
            keys = {(t, g) for t, g, _ in entries}
            hits = [h for h in hits if (h[1], h[2]) in keys][::3]
            assert len(hits) > 20
        table.update(PR.new_table(entries))
        PR.add_run(table, reads, hits, place(reads, hits), ALL)
        b = workspace(ix, reads)
        assert p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)[:2] == (len(hits), 0)
        b.close()
        if entries is not entries_a:
            ix.close()
    assert p.info()["n_segments"] == 3 and p.info()["n_refs"] == 10
    same(p, table, seq, DEFAULT, (1, 500000, 0, 1, 0), (2, 500000, 50000, 0, 100))
    keys = [r[:2] for r in row_tuples(p.consensus(*DEFAULT)[1])]
    assert keys == sorted(keys) and {(2, 25), (5, 1), (10, 10), (11, 20)} <= set(keys)
    assert keys.index((2, 21)) < keys.index((2, 25)) < keys.index((3, 30)) < keys.index((5, 1)) < keys.index((10, 10))
    text = p.consensus(*DEFAULT)[0].decode()
    assert [l[1:] for l in text.splitlines() if l.startswith(">")] == ["%d-%d" % (g, t) for t, g in keys]
    p.close()


# ---- 5. the accumulator is unchanged; add_counts merges pileups ----

def test_a_call_changes_nothing_and_two_calls_agree(crafted):
    ix, entries, reads, hits, place, table, _ = crafted
    keys = sorted(PL.seq_of(entries))
    b, p = workspace(ix, reads), M.Pileup(0)
    p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)
    sites_of = lambda: [(int(r["tax_id"]), int(r["gi"]), int(r["pos"]), int(r["ref"]), r["n"].tolist()) for r in p.sites(1, 1, 0)[0]]
    before, sites = state(p, keys), sites_of()
    first = p.consensus(*DEFAULT)
    second = p.consensus(*DEFAULT)
    assert first[0] == second[0] and first[1].tobytes() == second[1].tobytes() == p.consensus(*DEFAULT, fasta=False)[1].tobytes()
    assert state(p, keys) == before and sites_of() == sites and len(sites) > 100
    # a second accumulator takes the first's downloaded counters: equal to piling both runs into one
    q = M.Pileup(0)
    q.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)
    for key in keys:
        counts, _ = p.download(*key)
        q.add_counts(key[0], key[1], 0, counts, len(hits))
    p.add_run(b, PC.hits_array(hits, M.HIT_DTYPE), ALL)
    assert state(q, keys)[1] == state(p, keys)[1] and q.info()["hits_piled"] == (1 + len(keys)) * len(hits)
    assert q.consensus(*DEFAULT)[0] == p.consensus(*DEFAULT)[0] and q.consensus(*DEFAULT)[1].tobytes() == p.consensus(*DEFAULT)[1].tobytes()
    # a part of a reference, from a slot that is not its first: those slots hold four times the table, the others twice
    want = {k: [[2 * x for x in n] for n in v] for k, v in table.items()}
    counts, _ = p.download(2, 20)
    p.add_counts(2, 20, 1000, counts[1000:1600], 2 * len(hits))
    for k in range(1000, 1600):
        want[(2, 20)][k] = [2 * x for x in want[(2, 20)][k]]
    got, _ = p.download(2, 20)
    assert got.tolist() == want[(2, 20)]
    same(p, want, PL.seq_of(entries))
    for w in (q, p, b):
        w.close()


# ---- 6. refusals ----

def refused(call, code, *words):
    with pytest.raises(M.MtsvError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_accumulator_as_it_was(small, monkeypatch):
    ix, entries, *_ = small
    p, table = small_pileup(small)
    more = CC.random_tables(entries)
    add_table(p, more)
    CC.add_tables(table, more)
    keys = sorted(table)
    before = state(p, keys)
    one = np.zeros((1, 8), dtype=np.uint32)
    one[0, 0] = 5
    ins = np.zeros((1, 8), dtype=np.uint32)
    ins[0, 7] = 5
    cases = [
        (lambda: p.add_counts(9, 9, 0, one, 5), _lib.E_ARG, "holds no reference (tax_id 9, gi 9)"),
        (lambda: p.add_counts(1, 10, 0, one, 4), _lib.E_ARG, "a count of 5 at slot 0 with 4 hits"),
        (lambda: p.add_counts(1, 10, 62, one, 5), _lib.E_ARG, "slot L (62) takes insertions only"),
        (lambda: p.add_counts(1, 10, 63, ins, 5), _lib.E_ARG, "of a reference of 63 slots"),
        (lambda: p.add_counts(1, 10, 0, np.zeros((64, 8), dtype=np.uint32), 5), _lib.E_ARG, "of a reference of 63 slots"),
        (lambda: p.add_counts(1, 10, 0, one, (1 << 32) - 1 - before[0]["hits_piled"] + 1), _lib.E_LIMIT, "2^32 or more"),
        (lambda: p.consensus(1, 500000, 0, 2, 60), _lib.E_ARG, "fill of 2"),
        (lambda: p.consensus(1, 1000001, 0, 0, 60), _lib.E_ARG, "min_frac_ppm of 1000001"),
    ]
    for call, code, word in cases:
        refused(call, code, word)
        assert state(p, keys) == before
    fresh = M.Pileup(0)                                                        # (its arrays have never been allocated)
    b = workspace(ix, small[2])
    fresh.add_run(b, PC.hits_array(small[3], M.HIT_DTYPE), 0)
    b.close()
    for name, fasta in (("the consensus calls", True), ("the consensus calls", False), ("the consensus text", True)):
        monkeypatch.setenv("MTSV_ALLOC_REFUSE", name)
        refused(lambda: fresh.consensus(*DEFAULT, fasta=fasta), _lib.E_NOMEM, "no memory for " + name)
        monkeypatch.delenv("MTSV_ALLOC_REFUSE")
    monkeypatch.setenv("MTSV_ALLOC_REFUSE", "the consensus text")
    assert fresh.consensus(*DEFAULT, fasta=False)[0] is None                   # rows only: no text is allocated
    monkeypatch.delenv("MTSV_ALLOC_REFUSE")
    same(fresh, small[4], PL.seq_of(entries))
    p.add_counts(1, 10, 62, ins, 5)                                            # slot L takes an insertion
    table[(1, 10)][62][7] += 5
    same(p, table, PL.seq_of(entries), DEFAULT, (2, 0, 0, 1, 10))
    empty = M.Pileup(0)
    text, rows, ms = empty.consensus(*DEFAULT)                                 # no segment: nothing is launched
    assert (text, len(rows), ms) == (b"", 0, 0.0) and empty.consensus(*DEFAULT, fasta=False)[0] is None
    for w in (empty, fresh, p):
        w.close()


# ---- 7. mtsv-binner --fold-on-gpu --consensus, and the consensus built into an index ----

@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("cons_e2e")
    chunks = [PC.database(seed=5, first_tax=1), PL.second_chunk()]
    st = CC.strain(chunks[0])
    reads, ids = st["reads"], ["strain%d" % k for k in range(len(st["reads"]))]
    fq = d / "reads.fastq"
    with open(fq, "wb") as f:
        for r, i in zip(reads, ids):
            f.write(b"@" + i.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bases, off = helpers.reads_to_batch(reads)
    paths, runs = [], []
    place = PL.Placer(*chunks)
    for c, entries in enumerate(chunks):
        ix = M.MGIndex.build(entries, threads=4)
        paths.append(str(d / f"chunk{c}.idx"))
        ix.write(paths[-1])
        ix.to_device(0)
        b = M.Batch(ix, 0, len(reads), len(bases), lanes=1)
        b.upload(bases, off)
        b.run()
        hits = [tuple(int(h[k]) for k in ("read", "tax_id", "gi", "offset", "edit", "strand")) for h in b.download()]
        runs.append(hits)
        b.close()
        ix.close()

    def want(taxa, slack):
        table = {}
        for entries, hits in zip(chunks, runs):                                 # a call per chunk: the best edit is the chunk's
            table.update(PR.new_table(entries, taxa))
            PR.add_run(table, reads, hits, place(reads, hits), slack)
        return table

    return d, ",".join(paths), fq, want, PL.seq_of(*chunks), st


def binner(tmp_path, name, index, fq, *extra):
    res = tmp_path / f"{name}.res"
    r = subprocess.run([BINNER, *map(str, ["--fastq", fq, "-i", index, "-m", res, "--fold-on-gpu", "--batch-reads", "16", *extra])], capture_output=True,
                       text=True, timeout=600, env={**os.environ, "MTSV_CLI_TIMING": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    return res.read_bytes(), r.stderr


def test_binner_consensus_is_the_restatements_text_and_builds_into_an_index(e2e, tmp_path):
    d, index, fq, want, seq, st = e2e
    table = want(None, 0)
    var, var2, fa, tsv = tmp_path / "var.tsv", tmp_path / "var2.tsv", tmp_path / "cons.fa", tmp_path / "cons.tsv"
    plain, err = binner(tmp_path, "plain", index, fq, "--variants", var)
    assert len(plain) > 0 and "[cli consensus timing]" not in err
    res, err = binner(tmp_path, "cons", index, fq, "--variants", var2, "--consensus", fa, "--consensus-stats", tsv, "--consensus-min-depth", CC.STRAIN_DEPTH,
                      "--consensus-width", 60)
    want_text, want_rows = CR.consensus(table, seq, CC.STRAIN_DEPTH, 500000, 0, 0, 60)
    assert res == plain and var2.read_bytes() == var.read_bytes() == PR.text(PR.sites(table, seq, 1, 1, 0)).encode()
    assert fa.read_text() == want_text and tsv.read_text() == CR.stats_text(want_rows)
    assert "[cli consensus timing] hits piled " in err and "references %d, bytes %d;" % (len(want_rows), len(want_text)) in err
    key = st["key"]
    assert key in {r[:2] for r in want_rows} and ">%d-%d\n" % (key[1], key[0]) in want_text
    # --consensus alone makes the pileup too, and takes the pileup's flags; fractions as --min-alt-frac takes them
    res, _ = binner(tmp_path, "alone", index, fq, "--consensus", fa, "--variant-taxa", "%d,77" % key[0], "--variant-slack", "all", "--consensus-fill", "ref",
                    "--consensus-min-frac", "0.75", "--consensus-min-breadth", "0.1", "--consensus-width", "0")
    sub = want({key[0], 77}, ALL)
    assert res == plain and not (tmp_path / "alone.tsv").exists()
    assert fa.read_text() == CR.consensus(sub, seq, 1, 750000, 100000, 1, 0)[0] and fa.read_text().count(">") >= 1
    # the consensus of the sample as a database: mtsv-build reads the headers, and the index holds the consensus
    binner(tmp_path, "again", index, fq, "--consensus", fa, "--consensus-min-depth", CC.STRAIN_DEPTH, "--consensus-width", 60)
    assert fa.read_text() == want_text
    idx = tmp_path / "cons.idx"
    r = subprocess.run([BUILD, "-f", str(fa), "-i", str(idx), "--threads", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    ix = M.MGIndex.load(str(idx))
    ix.to_device(0)
    bins = np.frombuffer(ix.download_device(0, M.DEVPART_BINS), dtype="<u4").reshape(-1, 4)      # start, end, tax_id, gi
    text = np.frombuffer(ix.download_device(0, M.DEVPART_TEXT), dtype=np.uint8)
    assert sorted((int(b[2]), int(b[3])) for b in bins) == [r[:2] for r in want_rows]
    chars = CR.call_reference(table[key], seq[key], CC.STRAIN_DEPTH, 500000, 0)[0]
    start, end = next((int(b[0]), int(b[1])) for b in bins if (int(b[2]), int(b[3])) == key)
    assert end - start == len(chars) and np.minimum(text[start:end], 4).tolist() == [int(c) for c in R.codes(chars.encode())]
    ix.close()
