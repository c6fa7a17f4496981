"""No GPU: the kept levels of the k-mer table (dev_layout.hpp: kmer_level_start) as the general search kernel uses them
for a seed with an N in its table part.  The entry of level m of the m symbols behind the seed's last N (m capped at the
number of kept levels) is the interval of the plain backward search after those m symbols; stepping the remaining symbols
from there must end at the interval of the whole seed.  Here the entries come from the oracle's own search of the tail and
the remaining symbols are stepped with the oracle's Occ, on a database with N runs."""
import random

import pytest

import helpers
from oracle import oracle as O

LEVELS_MAX = 12  # dev_layout.hpp: kKmerLevelsMax


@pytest.fixture(scope="module")
def db():
    rng = random.Random(3)
    entries = []
    for tax in range(1, 9):
        body = bytearray(helpers.rnd_seq(rng, rng.randrange(1500, 2500)))
        for _ in range(4):  # N runs of 1..40
            p = rng.randrange(50, len(body) - 100)
            ln = rng.choice((1, 1, 2, 3, 8, 40))
            body[p:p + ln] = b"N" * ln
        entries.append((tax, 100 + tax, bytes(body)))
    entries.append((9, 200, b"ACGT" * 100))  # a repeat: wide intervals
    text = b"".join(e[2] for e in sorted(entries, key=lambda e: e[0]))
    return O.Index.build(entries), text


def less_of(orc, a):
    """less[a] of the oracle's index: the lower end of the one-symbol search (None when the symbol does not occur)"""
    ok, lo, _ = orc.backward_search(bytes([a]))
    return lo if ok else None


def step(orc, less, l, r, a):
    """one step of FMIndex::backward_search on the inclusive interval [l, r]"""
    if less[a] is None:
        return 1, 0
    L = O.lib()
    return (less[a] + (L.orc_occ_get(orc.h, l - 1, a) if l > 0 else 0), less[a] + L.orc_occ_get(orc.h, r, a) - 1)


def search_from_level(orc, less, seed, n_levels):
    """what search_slot does with a seed whose table part holds an N; None when it keeps the plain walk (m == 0)"""
    K = len(seed)
    m = 0
    while m < n_levels and m < K and seed[K - 1 - m] in b"ACGT":
        m += 1
    if m == 0:
        return None
    ok, lo, hi = orc.backward_search(seed[K - m:])  # the level entry: (0, 0) when the tail does not occur
    if not ok:
        return 0, 0
    l, r = lo, hi - 1
    for i in range(K - 1 - m, -1, -1):
        l, r = step(orc, less, l, r, seed[i])
        if l == r + 1:
            return 0, 0
    return l, r + 1


def seeds_with_n(rng, text, K):
    """seeds of K symbols cut from the text (they occur) and altered ones (mostly absent): an N at every position, two N,
    N at both ends, and seeds over the text's own N runs and their flanks"""
    out = []
    for pos in range(K):
        for _ in range(6):
            st = rng.randrange(0, len(text) - K)
            s = bytearray(text[st:st + K])
            s[pos] = ord("N")
            out.append(bytes(s))
            s2 = bytearray(s)
            s2[rng.randrange(K)] = ord("N")
            out.append(bytes(s2))
    for _ in range(20):
        st = rng.randrange(0, len(text) - K)
        s = bytearray(text[st:st + K])
        s[0] = s[-1] = ord("N")
        out.append(bytes(s))
    at = 0
    while True:  # every window that overlaps an N of the text
        at = text.find(b"N", at)
        if at < 0:
            break
        for st in range(max(0, at - K + 1), min(at + 1, len(text) - K + 1)):
            out.append(text[st:st + K])
        at += 1
    out.append(b"N" * K)
    out.append((b"N" + b"ACGT" * 8)[:K])
    return out


@pytest.mark.parametrize("K", [16, 18, 21, 24])
def test_level_entry_then_remaining_steps_equals_plain_search(db, K):
    orc, text = db
    rng = random.Random(K)
    less = {a: less_of(orc, a) for a in b"ACGTN"}
    n_from_level = n_found = 0
    for kmer_k in (8, 12, 16, 17):
        n_levels = min(kmer_k, LEVELS_MAX)
        for seed in seeds_with_n(rng, text, K):
            assert b"N" in seed
            got = search_from_level(orc, less, seed, n_levels)
            if got is None:
                assert seed[-1:] == b"N"
                continue
            ok, lo, hi = orc.backward_search(seed)
            assert got == (lo, hi), (seed, kmer_k)
            n_from_level += 1
            n_found += ok
    assert n_from_level > 1000 and n_found > 50
