"""-m gpu: singleton k-mers of the table carry their text position (dev_layout.hpp, kKmerTag).  A seed that finds
such an entry is resolved without rank steps or an SA gather; hits and counters must be exactly those of the
untagged table (MTSV_KMER_POS=0) and of the CPU oracle."""
import random
import re

import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STATS = ("n_seed_hits", "n_candidates", "n_verified", "window_bytes", "n_hits")
ORACLE_KEY = {"n_seed_hits": "H", "n_candidates": "n_cand", "n_verified": "n_sw", "window_bytes": "W", "n_hits": "R"}

# table width -> seed parameters; every (width, seed) pair of test_kmer_table_width_does_not_change_hits for widths
# 12..17, plus seeds that leave 3..8 front symbols to the fast kernel's text comparison
WIDTHS = {
    "17": [{}, dict(seed_size=17, seed_interval=9), dict(seed_size=25), dict(seed_size=16, seed_interval=7),
           dict(seed_size=20), dict(seed_size=24, seed_interval=11)],
    "16": [{}, dict(seed_size=24, seed_interval=11), dict(seed_size=16, seed_interval=7), dict(seed_size=19)],
    "15": [{}, dict(seed_size=20)],
    "14": [{}, dict(seed_size=22)],
    "13": [{}, dict(seed_size=22)],
    "12": [{}, dict(seed_size=20)],
}


def both_params(**over):
    mp = M.default_params(**over)
    op = O.default_params(**over)
    return mp, op


def tagged_entries(text):
    m = re.findall(r"\[upload\] kmer table k=(\d+): (\d+) tagged entries", text)
    assert m, text[-2000:]
    return int(m[-1][1])


def upload(entries, monkeypatch, capfd, kmer_pos, k=None, flags=M.DEV_DEFAULT):
    """A fresh index on device 0 (MTSV_KMER_POS is read at upload); returns it and the number of tagged entries."""
    ix = M.MGIndex.build(entries, threads=4)
    monkeypatch.setenv("MTSV_TRACE", "1")
    if k:
        monkeypatch.setenv("MTSV_KMER_K", k)
    if not kmer_pos:
        monkeypatch.setenv("MTSV_KMER_POS", "0")
    capfd.readouterr()
    ix.to_device(0, flags)
    n_tagged = tagged_entries(capfd.readouterr().err)
    for v in ("MTSV_TRACE", "MTSV_KMER_K", "MTSV_KMER_POS"):
        monkeypatch.delenv(v, raising=False)
    return ix, n_tagged


def run(ix, batch, mp, generic=False, monkeypatch=None):
    """One Batch over (bases, off); generic: every seed slot through the general search kernel."""
    bases, off = batch
    b = M.Batch(ix, 0, len(off) - 1, max(len(bases), 1))
    b.upload(bases, off)
    if generic:
        monkeypatch.setenv("MTSV_SEARCH_GENERIC", "1")
    b.run(mp)
    if generic:
        monkeypatch.delenv("MTSV_SEARCH_GENERIC")
    hits, st = b.download(), b.stats()
    b.close()
    return hits, st


@pytest.fixture(scope="module")
def tricky_set(tmp_path_factory):
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.close()
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=30, lengths=(100, 150, 253))
    reads += edge_reads(entries)
    return entries, O.Index.read(p), helpers.reads_to_batch(reads)


def index_text(entries):
    """The index's text: the sequences in ascending TaxId order (stable), DNA5-normalised (builder.cpp)."""
    raw = b"".join(e[2] for e in sorted(entries, key=lambda e: e[0])).upper()
    return bytes(c if c in b"ACGTN" else ord("N") for c in raw)


def edge_reads(entries, seed=5):
    """Reads whose first seed has its k-mer at the very start of the text behind 1..8 extra symbols, so that the
    k-mer sits at p < m (m = the seed's symbols in front of the table part), and reads whose seeds have an N run
    right in front of their k-mer (front symbols N against N in the text)."""
    rng = random.Random(seed)
    out = []
    text = index_text(entries)
    for extra in range(1, 9):
        for _ in range(3):
            r = helpers.rnd_seq(rng, extra) + text[:150 - extra]
            out += [r, helpers.revcomp(r)]
    for t in (e[2].upper() for e in entries if len(e[2]) >= 200):
        for run in re.finditer(rb"N+", t):
            e = run.end()  # first base after the run
            for back in range(1, 9):
                for gap in (0, 15, 30):
                    st = e - back - gap
                    if st < 0 or st + 150 > len(t):
                        continue
                    r = t[st:st + 150]
                    out += [r, helpers.revcomp(r)]
    return out


def seeds_before_text_start(entries, K, k):
    """How many of the extra-symbol counts 1..8 of edge_reads give the read's first seed (K symbols, table of k) a
    singleton ACGT k-mer at text position p < m: the case whose front symbols would lie before the text."""
    text = index_text(entries)
    m = K - k
    n = 0
    for extra in range(1, min(m, 8) + 1):
        p = m - extra
        kmer = text[p:p + k]
        if all(c in b"ACGT" for c in kmer) and len(re.findall(b"(?=" + kmer + b")", text)) == 1:
            n += 1
    return n


def test_edge_reads_reach_the_start_of_the_text():
    """(CPU-side check of the inputs) the p < m case occurs for every table/seed pair below that leaves front
    symbols, including pairs whose m >= 3 takes the text comparison."""
    entries, _, _ = helpers.tricky_db(seed=7)
    default_K = O.default_params().seed_size
    for k, sets in WIDTHS.items():
        for extra in sets:
            K = extra.get("seed_size", default_K)
            if K > int(k):
                assert seeds_before_text_start(entries, K, int(k)) > 0, (k, K)


@pytest.mark.parametrize("k", list(WIDTHS))
def test_tagged_table_gives_identical_hits_and_counters(tricky_set, monkeypatch, capfd, k):
    entries, orc, batch = tricky_set
    results = {}
    for pos in (False, True):
        ix, n_tagged = upload(entries, monkeypatch, capfd, pos, k=k)
        assert (n_tagged > 0) == pos, n_tagged
        for i, extra in enumerate(WIDTHS[k]):
            mp, _ = both_params(**extra)
            results[pos, i] = run(ix, batch, mp, monkeypatch=monkeypatch)
            results[pos, i, "generic"] = run(ix, batch, mp, generic=True, monkeypatch=monkeypatch)
        ix.close()
    for i, extra in enumerate(WIDTHS[k]):
        _, op = both_params(**extra)
        want, ctr = orc.bin_batch(*batch, op, threads=8)
        assert len(want) > 50
        for key in [(False, i), (True, i), (False, i, "generic"), (True, i, "generic")]:
            hits, st = results[key]
            assert_same_hits(hits, want)
            for s in STATS:
                assert st[s] == ctr[ORACLE_KEY[s]], (key, extra, s)
                assert st[s] == results[False, i][1][s], (key, extra, s)


def test_default_params_on_synth_db(monkeypatch, capfd, tmp_path):
    src = M.MGIndex.synth(seed=21, n_taxa=16, gis_per_taxon=4, seq_len=5000)
    p = str(tmp_path / "synth.idx")
    src.write(p)
    bases, off = M.synth_reads(src, seed=155, n_reads=4000, read_len=150)
    orc = O.Index.read(p)
    want, ctr = orc.bin_batch(bases, off, O.default_params(), threads=8)
    assert len(want) > 1000
    got = {}
    for pos in (False, True):
        ix = M.MGIndex.load(p)
        monkeypatch.setenv("MTSV_TRACE", "1")
        if not pos:
            monkeypatch.setenv("MTSV_KMER_POS", "0")
        capfd.readouterr()
        ix.to_device(0)
        n_tagged = tagged_entries(capfd.readouterr().err)
        monkeypatch.delenv("MTSV_TRACE")
        monkeypatch.delenv("MTSV_KMER_POS", raising=False)
        assert (n_tagged > 0) == pos, n_tagged
        got[pos] = run(ix, (bases, off), M.default_params())
        ix.close()
    for pos in (False, True):
        hits, st = got[pos]
        assert_same_hits(hits, want)
        for s in STATS:
            assert st[s] == ctr[ORACLE_KEY[s]] == got[False][1][s], (pos, s)
    src.close()


def test_sampled_sa_keeps_lf_walk(tricky_set, monkeypatch, capfd):
    """The sampled-SA mode is not tagged: its locate still walks LF exactly as far as the reference does."""
    entries, orc, batch = tricky_set
    ix, n_tagged = upload(entries, monkeypatch, capfd, True, flags=M.DEV_SAMPLED_SA_ONLY)
    assert n_tagged == 0
    hits, st = run(ix, batch, M.default_params())
    ix.close()
    want, ctr = orc.bin_batch(*batch, O.default_params(), threads=8)
    assert_same_hits(hits, want)
    assert st["lf_steps"] == ctr["S"] > 0
    for s in STATS:
        assert st[s] == ctr[ORACLE_KEY[s]], s
