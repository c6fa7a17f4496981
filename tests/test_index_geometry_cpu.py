"""The index geometry ladder (helpers.RUNGS) on the host: the oracle is pinned against brute force on every rung before
the device is compared with it, and the product's host builder must write the oracle's bytes on every rung.  No GPU."""
import random

import pytest

import helpers
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib
from oracle import oracle as O

BRUTE_MAX_N = 131073


def test_the_ladder_is_what_it_says():
    """every rung's text has exactly n symbols, the sentinel-row rungs sit where they claim (the search for them is
    bounded and asserts that it found all seven), and the sizes straddle the branches they are there for"""
    seeds = helpers.sentinel_seeds()
    assert set(seeds) == set(helpers.SENTINEL_TARGETS)
    for t, (_, row) in seeds.items():
        if t.startswith("res"):
            assert row % 128 == int(t[3:])
    assert seeds["first_block"][1] < 128 and seeds["last_block"][1] >= 4096 - 128
    for r in helpers.RUNGS:
        entries = r.entries()
        assert sum(len(e[2]) for e in entries) + 1 == r.n
        assert [e[0] for e in entries] == sorted(e[0] for e in entries)  # the entries' order is the text's order
        if r.kind != "tinybins" and r.n > 1:
            assert any(len(e[2]) == 0 for e in entries)
    w = helpers.kmer_width_for
    assert (w(1), w(7), w(8), w(32767), w(32768), w(65537)) == (1, 1, 2, 7, 8, 8)
    assert ((524159 >> 7) + 1, (524160 >> 7) + 1) == (4095, 4096)
    assert len(helpers.RUNGS) == 110


def _patterns(rng, text):
    L = len(text)
    pats = set()
    if L >= 18:
        starts = range(L - 17) if L - 17 <= 400 else [0, L - 18] + [rng.randrange(L - 17) for _ in range(600)]
        for i in starts:
            pats.add(text[i:i + 18])
            if len(pats) >= 400:
                break
    at_n = [i for i in range(L) if text[i] == 78 and (i == 0 or text[i - 1] != 78 or i + 1 == L or text[i + 1] != 78)]
    for i in at_n[:40]:  # the edges of the N runs: patterns that hold 1..18 N
        for back in (0, 5, 17):
            s = max(0, i - back)
            pats.add(text[s:s + 18])
    pats.discard(b"")
    pats = sorted(pats)
    pats += [b"A", b"C", b"G", b"T", b"N"]
    absent, tries = [], 0
    while len(absent) < 20 and tries < 2000:
        tries += 1
        p = helpers.rnd_seq(rng, rng.randrange(10, 19))
        if p not in text:
            absent.append(p)
    assert len(absent) == 20
    return pats + absent, absent


@pytest.mark.parametrize("rung", [r for r in helpers.RUNGS if r.n <= BRUTE_MAX_N], ids=repr)
def test_oracle_search_and_locate_equal_brute_force(rung):
    """test_fm_search_and_locate_equal_brute_force on every rung: backward_search's interval and sa_get's positions
    against a plain scan of the text"""
    entries = rung.entries()
    text = helpers.geometry_text(entries)
    ix = O.Index.build(entries, rung.occ_k, rung.sa_s)
    pats, absent = _patterns(random.Random(rung.n), text)
    for pat in pats:
        ok, lo, hi = ix.backward_search(pat)
        brute = sorted(ix.brute_find(pat, cap=rung.n + 1).tolist())
        if rung.n < 5000:  # (and the scan itself against Python's)
            assert brute == [i for i in range(len(text) - len(pat) + 1) if text.startswith(pat, i)], pat
        if not brute:
            assert not ok and lo == hi == 0, (pat, lo, hi)
            continue
        assert pat not in absent
        assert ok and hi - lo == len(brute), (pat, lo, hi, len(brute))
        assert sorted(ix.sa_get(r) for r in range(lo, hi)) == brute, pat


@pytest.mark.parametrize("rung", helpers.RUNGS, ids=repr)
def test_host_builder_writes_the_oracles_bytes(rung, tmp_path):
    """MGIndex.build(...).write against the oracle's builder, byte for byte, and the loader reads back what was written.
    A rung that one of them refuses must be refused by both, by the product with an error code and a message."""
    entries = rung.entries()
    a, b, c = (str(tmp_path / x) for x in ("a.idx", "b.idx", "c.idx"))
    try:
        O.Index.build(entries, rung.occ_k, rung.sa_s).write(b)
        oracle_refuses = False
    except RuntimeError:
        oracle_refuses = True
    try:
        M.MGIndex.build(entries, rung.occ_k, rung.sa_s, threads=3).write(a)
        product_refuses = False
    except M.MtsvError as e:
        product_refuses = True
        assert e.code in (_lib.E_FORMAT, _lib.E_LIMIT) and len(str(e)) > len("mtsv error -3: "), e
    assert product_refuses == oracle_refuses
    if product_refuses:
        return
    assert open(a, "rb").read() == open(b, "rb").read()
    back = M.MGIndex.load(a)
    info = back.info()
    assert info["n"] == rung.n and info["occ_k"] == rung.occ_k and info["sa_s"] == rung.sa_s
    assert info["n_bins"] == len(entries)
    back.write(c)
    assert open(c, "rb").read() == open(a, "rb").read()
    O.Index.read(a).write(c)
    assert open(c, "rb").read() == open(a, "rb").read()


def _derived_n_rank_model(text, sentinel_before_block):
    """backward search over rank blocks of 128 rows as dev_layout.hpp lays them out, in plain Python: A, C, G, T counted,
    the rank of N derived -- rows before the block minus A+C+G+T before it minus one if the sentinel lies before the block,
    which sentinel_before_block(first row of the block, sentinel row) decides"""
    order = b"$ACGNT"
    text = text + b"$"
    n = len(text)
    sa = sorted(range(n), key=lambda i: text[i:])
    bwt = bytes(text[i - 1] for i in sa)
    srow = sa.index(0)
    less = {c: sum(1 for x in text if order.index(x) < order.index(c)) for c in order}
    pref = {c: [0] * (n + 1) for c in b"ACGT"}
    for c in b"ACGT":
        for i, x in enumerate(bwt):
            pref[c][i + 1] = pref[c][i] + (x == c)

    def rank(c, pos):
        if c != 78:
            return pref[c][pos]
        before = (pos >> 7) << 7
        base = before - sum(pref[a][before] for a in b"ACGT") - (1 if sentinel_before_block(before, srow) else 0)
        return base + bwt.count(b"N", before, pos)

    def search(pat):
        lo, hi = 0, n
        for c in reversed(pat):
            lo, hi = less[c] + rank(c, lo), less[c] + rank(c, hi)
            if lo >= hi:
                return 0, 0
        return lo, hi

    return srow, search


@pytest.mark.parametrize("rung", [r for r in helpers.RUNGS if r.kind == "sentinel"], ids=repr)
def test_n_probes_read_the_derived_rank_of_n_where_the_sentinel_row_decides_it(rung):
    """The N probes of the GPU file on a model of block_rank: with the comparison as it is (before > sentinel_row) the
    model gives the oracle's interval for every seed of every probe; with >= instead, which differs only in the block
    whose first row is the sentinel row, it gives another interval for at least one seed of the residue-0 rung.  So
    that rung's probes do read the rank that the comparison decides."""
    entries = rung.entries()
    text = helpers.geometry_text(entries)
    orc = O.Index.build(entries, rung.occ_k, rung.sa_s)
    srow, good = _derived_n_rank_model(text, lambda before, s: before > s)
    _, bad = _derived_n_rank_model(text, lambda before, s: before >= s)
    assert srow == rung.sentinel_row()
    seeds = set()
    for rd in helpers.n_edge_probes(random.Random(rung.n + 2), text):
        for s in (rd, helpers.revcomp(rd)):
            seeds.update(s[off:off + 18] for off in range(0, len(s) + 1 - 18, 15))
    assert any(1 <= s.count(b"N") < 18 for s in seeds)
    for s in seeds:
        ok, lo, hi = orc.backward_search(s)
        assert good(s) == (lo, hi), s
    changed = sum(1 for s in seeds if good(s) != bad(s))
    assert (changed > 0) == (rung.target == "res0"), changed
