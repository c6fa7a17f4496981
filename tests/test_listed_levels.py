"""-m gpu: seeds with an N in their table part start from a kept level of the k-mer table (dev_layout.hpp:
kmer_level_start) instead of walking their N-free tail a rank step per symbol.  Batches in which every read has an N in
some seed -- reads with planted N, reads cut from the text's own N runs and their flanks -- must give the oracle's hits and
counters for every table width, with and without the levels (MTSV_KMER_LEVELS=0), for seed sizes on the fast, the listed
and the general search kernel, and when the listed kernel's grid overflows and the pass runs again."""
import random
import re

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
from helpers import assert_same_hits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STATS = {"n_seed_hits": "H", "n_candidates": "n_cand", "n_verified": "n_sw", "window_bytes": "W", "n_hits": "R"}
# seed parameters: the default (18 on the fast kernel + the listed one), others on it, and 25 / 30, which the general
# kernel takes for every table width here (more than 8 symbols in front of the table part)
SEEDS = [{}, dict(seed_size=16, seed_interval=7), dict(seed_size=21), dict(seed_size=24, seed_interval=11),
         dict(seed_size=25), dict(seed_size=30, seed_interval=9)]


def both_params(**over):
    return M.default_params(**over), O.default_params(**over)


def levels_kept(text):
    m = re.findall(r"\[upload\] kmer levels 1\.\.(\d+) kept: (\d+) bytes", text)
    assert m, text[-2000:]
    return int(m[-1][0]), int(m[-1][1])


def upload(entries, monkeypatch, capfd, k=None, levels=True):
    """A fresh index on device 0 (the table's environment is read at upload); returns it and (levels, bytes) kept."""
    ix = M.MGIndex.build(entries, threads=4)
    monkeypatch.setenv("MTSV_TRACE", "1")
    if k:
        monkeypatch.setenv("MTSV_KMER_K", k)
    if not levels:
        monkeypatch.setenv("MTSV_KMER_LEVELS", "0")
    capfd.readouterr()
    ix.to_device(0)
    kept = levels_kept(capfd.readouterr().err)
    for v in ("MTSV_TRACE", "MTSV_KMER_K", "MTSV_KMER_LEVELS"):
        monkeypatch.delenv(v, raising=False)
    return ix, kept


def n_reads(entries, seed=19):
    """reads of 100..253 bases, each with an N in some seed: one or two N planted in a read from the text (at the very
    end, the very start, anywhere), a few edits besides; and reads over the text's N runs and their flanks"""
    rng = random.Random(seed)
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    out = []
    for i in range(1500):
        t = rng.choice(texts)
        L = rng.choice((100, 150, 150, 253))
        st = rng.randrange(0, len(t) - L)
        r = bytearray(helpers.mutate(rng, t[st:st + L], rng.choice((0, 0, 1, 3)), b"ACGT")[:L])
        for _ in range(rng.choice((1, 1, 2, 4))):
            r[rng.choice((0, len(r) - 1, rng.randrange(len(r)), rng.randrange(len(r))))] = ord("N")
        out.append(bytes(r) if i % 2 else helpers.revcomp(bytes(r)))
    for t in texts:
        for run in re.finditer(rb"N+", t):
            for edge in (run.start(), run.end()):
                for back in (1, 2, 5, 11, 12, 13, 16, 17, 18, 40, 149):
                    st = edge - back
                    if st < 0 or st + 150 > len(t):
                        continue
                    r = t[st:st + 150]
                    out += [r, helpers.revcomp(r)]
    assert all(b"N" in r for r in out)
    return out


@pytest.fixture(scope="module")
def n_set(tmp_path_factory):
    entries, _, _ = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    p = str(tmp_path_factory.mktemp("idx") / "tricky.idx")
    ix.write(p)
    ix.close()
    return entries, O.Index.read(p), helpers.reads_to_batch(n_reads(entries))


def run(ix, batch, mp):
    bases, off = batch
    b = M.Batch(ix, 0, len(off) - 1, max(len(bases), 1))
    b.upload(bases, off)
    b.run(mp)
    hits, st = b.download(), b.stats()
    b.close()
    return hits, st


@pytest.mark.parametrize("k", ["8", "12", "13", "16"])
def test_levels_give_the_oracles_hits_and_counters(n_set, monkeypatch, capfd, k):
    entries, orc, batch = n_set
    results = {}
    for levels in (False, True):
        ix, (n_levels, n_bytes) = upload(entries, monkeypatch, capfd, k=k, levels=levels)
        want_levels = min(int(k), 12) if levels else 0
        assert n_levels == want_levels
        assert n_bytes == (8 * (4 ** (want_levels + 1) - 4) // 3 if levels else 0)
        for i, extra in enumerate(SEEDS):
            results[levels, i] = run(ix, batch, both_params(**extra)[0])
        ix.close()
    for i, extra in enumerate(SEEDS):
        want, ctr = orc.bin_batch(*batch, both_params(**extra)[1], threads=8)
        assert len(want) > 200
        for levels in (False, True):
            hits, st = results[levels, i]
            assert_same_hits(hits, want)
            for s, o in STATS.items():
                assert st[s] == ctr[o], (levels, extra, s)


def test_device_bytes_grow_by_the_levels(n_set, monkeypatch, capfd):
    entries, _, _ = n_set
    sizes = {}
    for levels in (False, True):
        ix, kept = upload(entries, monkeypatch, capfd, k="13", levels=levels)
        sizes[levels] = ix.info()["device_bytes"], kept[1]
        ix.close()
    assert sizes[True][1] == 8 * (4 ** 13 - 4) // 3
    assert sizes[True][0] - sizes[False][0] == sizes[True][1]


def test_n_rich_batches_that_overflow_the_listed_grid(monkeypatch, capfd, tmp_path):
    """an N every dozen bases: three seeds in four go to the list, the listed kernel's grid (sized from the passes before)
    is too small, and the pass runs again -- from the levels both times"""
    src = M.MGIndex.synth(seed=21, n_taxa=16, gis_per_taxon=4, seq_len=5000)
    p = str(tmp_path / "small.idx")
    src.write(p)
    orc = O.Index.read(p)
    rng = np.random.default_rng(3)
    clean, off = M.synth_reads(src, seed=77, n_reads=6000, read_len=150)
    dirty = clean.copy()
    dirty[rng.random(len(dirty)) < 0.08] = ord("N")
    mp, op = both_params(edit_rate=0.2)
    want_dirty, ctr = orc.bin_batch(dirty, off, op, threads=8)
    want_clean, _ = orc.bin_batch(clean, off, op, threads=8)
    assert len(want_dirty) > 100 and len(want_clean) > 4000
    monkeypatch.setenv("MTSV_TRACE", "1")
    monkeypatch.setenv("MTSV_KMER_K", "12")   # (the table this small index would get by itself is too narrow for the fast kernel and its list)
    capfd.readouterr()
    src.to_device(0)
    monkeypatch.delenv("MTSV_KMER_K")
    assert levels_kept(capfd.readouterr().err)[0] == 12
    b = M.Batch(src, 0, 6000, len(clean))
    again = 0
    for bases, want in ((dirty, want_dirty), (clean, want_clean), (clean, want_clean), (dirty, want_dirty)):
        b.upload(bases, off)
        b.run(mp)
        again += capfd.readouterr().err.count("pass again")
        assert_same_hits(b.download(), want)
    assert again >= 1
    st = b.stats()
    assert st["n_seed_hits"] == ctr["H"] and st["n_candidates"] == ctr["n_cand"]
    b.run_host(dirty, off, mp)
    assert_same_hits(b.download(), want_dirty)
    b.close()
    src.close()
