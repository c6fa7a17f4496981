"""The cases of test_coverage_cpu.py and test_coverage.py: tables of references (tax_id, gi, length), folds as lists of
(read, tax_id, gi, offset, edit) ordered by that key with distinct (read, tax_id, gi, offset), and the reads' lengths.  A
case is (refs, [(recs, read_len), ..]); nothing here comes from the device."""
import random
import re

import numpy as np

BIG = 0x80000005  # a TaxID of 2^31 or more


def as_array(recs, dtype):
    a = np.zeros(len(recs), dtype=dtype)
    for k, name in enumerate(("read", "tax_id", "gi", "offset", "edit")):
        a[name] = [r[k] for r in recs]
    return a


def words_of(offset, read_len, length):
    """the 64-bit words of a reference that the interval [offset, min(offset + read_len, length)) touches"""
    end = min(offset + read_len, length)
    return 0 if end <= offset else (end - 1) // 64 - offset // 64 + 1


def one_read_each(hits, edit=0, gaps=()):
    """hits: (tax_id, gi, offset, read_len), one read each, numbered in this order; gaps: reads (by number) left without a record"""
    recs, read_len = [], []
    for t, g, o, n in hits:
        while len(read_len) in gaps:
            read_len.append(77)
        recs.append((len(read_len), t, g, o, edit))
        read_len.append(n)
    return recs, read_len


EDGE_REFS = [(5, 1, 1), (5, 2, 63), (5, 3, 64), (5, 4, 65), (5, 5, 128), (5, 6, 4097),   # adjacent in the table
             (6, 1, 65), (6, 2, 1),                                                        # bits at the end of the first must not leak
             (7, 1, 0), (7, 2, 70),                                                        # a reference without a base owns no word
             (BIG, 7, 300)]


def edges():
    hits = [
        (5, 6, 64, 64), (5, 6, 128, 128),                     # start and end on word boundaries: one word, two words
        (5, 6, 63, 2), (5, 6, 65, 63), (5, 6, 191, 1), (5, 6, 192, 1),  # one base before and after a boundary
        (5, 6, 300, 130), (5, 6, 1000, 520),                  # three words, nine words
        (5, 6, 4090, 100), (5, 6, 4096, 50),                  # clamped at L, and starting at L - 1
        (5, 1, 0, 10), (5, 2, 60, 10), (5, 3, 0, 64), (5, 4, 64, 5), (5, 5, 127, 1),
        (5, 5, 10, 0),                                        # a read of no base: an alignment of 0 bases
        (6, 1, 60, 100), (6, 1, 64, 1),                       # the last five bases and the last base of a reference of 65
        (7, 2, 0, 70),
        (BIG, 7, 0, 300),                                     # the last reference of the table
    ]
    assert [words_of(o, n, 4097) for t, g, o, n in hits[:10]] == [1, 2, 2, 1, 1, 1, 3, 9, 2, 1]
    recs, read_len = one_read_each(hits, gaps=(3, 11))
    read_len.append(50)                                       # ... and the last read has none either
    return EDGE_REFS, [(recs, read_len)]


SLACK_REFS = [(10, 1, 1000), (10, 2, 1000)]


def slack():
    recs = [(0, 10, 1, 0, 0), (0, 10, 1, 100, 1), (0, 10, 1, 200, 3), (0, 10, 2, 0, 1), (0, 10, 2, 50, 3),
            (1, 10, 1, 500, 2), (1, 10, 2, 500, 4), (1, 10, 2, 600, 5)]
    return SLACK_REFS, [(recs, [80, 120])]


TIER_REF = (20, 1, 100000)


def tiers():
    """intervals of exactly k and k + 1 words for k in 0, 2, 8, and reads of 150, 600 and 32,767 bases"""
    hits = []
    for j, k in enumerate((0, 2, 8)):
        at = 64 * 100 * (j + 1)
        hits.append((20, 1, at, 64 * k))
        hits.append((20, 1, at + 64 * 40 + 63, 64 * (k - 1) + 2 if k else 1))
    hits += [(20, 1, 10, 150), (20, 1, 30000, 600), (20, 1, 40063, 32767)]
    spans = [words_of(o, n, TIER_REF[2]) for t, g, o, n in hits]
    assert spans == [0, 1, 2, 3, 8, 9, 3, 11, 513], spans
    recs, read_len = one_read_each(hits)
    return [TIER_REF], [(recs, read_len)], spans


def pop_tiles():
    """200 references of one word, then one of 100,000 bases: at tiles of 64 words many references per tile, and one reference
    over 25 tiles; intervals on both sides of the tiles' edges"""
    refs = [(30, g, 1 + (g * 37) % 64) for g in range(1, 201)] + [(31, 1, 100000)]
    hits = [(30, g, 0, 100) for g in range(1, 201) if g % 3] + [(30, 64, 0, 1), (30, 65, 0, 1), (30, 128, 0, 2)]
    for tile in range(4, 25, 3):                     # the big reference begins at word 200: word 64 * tile is its base ...
        edge = (64 * tile - 200) * 64
        hits += [(31, 1, edge - 90, 150), (31, 1, edge - 1, 1), (31, 1, edge, 1)]
    hits += [(31, 1, 0, 150), (31, 1, 99990, 150), (31, 1, 50000, 5000)]
    hits = sorted(set(hits))
    recs, read_len = one_read_each(hits)
    return refs, [(recs, read_len)]


def hot_locus(seed=11):
    """5,000 reads with one and the same interval among 2,000 ordinary reads"""
    rng = random.Random(seed)
    refs = [(40, 1, 5000), (40, 2, 50000)]
    kinds = [True] * 5000 + [False] * 2000
    rng.shuffle(kinds)
    hits = [(40, 1, 1000, 150) if hot else (40, 2, rng.randrange(0, 50000), 150) for hot in kinds]
    return refs, [one_read_each(hits)]


def random_refs(rng, n_refs):
    refs = {}
    while len(refs) < n_refs:
        t = rng.choice([3, 9, 17, 400, 401, BIG, BIG + 9])
        g = rng.randrange(1, 200)
        refs[(t, g)] = rng.choice([0, 1, 63, 64, 65, 200, 1000, rng.randrange(1, 5000), rng.randrange(1, 70000)])
    return [(t, g, n) for (t, g), n in sorted(refs.items())]


def random_fold(rng, refs, n_reads, per_read=12):
    """a fold of n_reads reads on the references that have a base"""
    live = [r for r in refs if r[2] > 0]
    recs, read_len = [], []
    for r in range(n_reads):
        read_len.append(rng.choice([0, 50, 100, 150, 300, rng.randrange(1, 2000)]))
        keys = set()
        for _ in range(rng.choice([0, 1, 1, 2, 3, per_read, rng.randrange(0, 2 * per_read)])):
            t, g, n = rng.choice(live[:12]) if rng.random() < 0.5 else rng.choice(live)
            keys.add((t, g, rng.randrange(0, n)))
        recs += [(r, t, g, o, rng.randrange(0, 6)) for t, g, o in sorted(keys)]
    return recs, read_len


def random_case(seed=3, n_reads=2000, n_refs=300):
    rng = random.Random(seed)
    refs = random_refs(rng, n_refs)
    return refs, [random_fold(rng, refs, n_reads)]


# ---- end to end: reads tiled along a stretch of one bin of a synthetic chunk ----

READ_LEN, STEP = 100, 50


def n_free_stretch(index_file, bin_no=0, at_most=6000):
    """(the bin, s, e): the beginning of the longest stretch without N of a bin, in the bin's own coordinates"""
    b = index_file.bins[bin_no]                              # (gi, tax_id, start, end)
    text = index_file.text[b[2]:b[3]]
    s, e = max(((m.start(), m.end()) for m in re.finditer(rb"[ACGT]+", text)), key=lambda x: x[1] - x[0])
    return b, s, min(e, s + at_most)


def tiled_reads(index_file, bin_no=0):
    """reads of READ_LEN bases cut every STEP bases along the stretch; they lie inside it"""
    b, s, e = n_free_stretch(index_file, bin_no)
    text = index_file.text[b[2]:b[3]]
    return b, s, e, [text[o:o + READ_LEN] for o in range(s, e - READ_LEN + 1, STEP)]


def untouched_refs(index_file, b):
    """the references of the last bin's taxon, when it is not the stretch's: no read of e2e_reads is cut from them"""
    last = index_file.bins[-1]
    assert last[1] != b[1]
    return [(x[1], x[0]) for x in index_file.bins if x[1] == last[1]]


def e2e_reads(index_file, seed=7, n_scattered=250, n_random=20, n_copies=30):
    """the tiled reads, reads cut from other bins (not of the last bin's taxon), random reads, and copies of some of them;
    an even number, shuffled"""
    rng = random.Random(seed)
    b, s, e, reads = tiled_reads(index_file)
    last_taxon = index_file.bins[-1][1]
    bins = [x for x in index_file.bins[1:] if x[1] != last_taxon]
    while len(reads) < (e - s - READ_LEN) // STEP + 1 + n_scattered:
        x = rng.choice(bins)
        o = rng.randrange(x[2], x[3] - READ_LEN)
        if b"N" not in index_file.text[o:o + READ_LEN]:
            reads.append(index_file.text[o:o + READ_LEN])
    reads += [bytes(rng.choice(b"ACGT") for _ in range(READ_LEN)) for _ in range(n_random)]
    reads += [rng.choice(reads) for _ in range(n_copies)]
    if len(reads) & 1:
        reads.append(reads[0])
    rng.shuffle(reads)
    return b, s, e, reads


def condition(rows, b, s, e, other_taxon_refs):
    """what the end-to-end runs are held to: the stretch is covered but for the last 100 bases, and a reference of another
    taxon that no read was cut from is covered less; rows: (tax_id, gi, length, reads, alignments, bases, covered)"""
    by_ref = {(r[0], r[1]): r for r in rows}
    mine = by_ref[(b[1], b[0])]
    assert mine[6] >= (e - s) - READ_LEN, (mine, s, e)
    breadth = lambda r: r[6] / r[2]
    for key in other_taxon_refs:
        assert breadth(by_ref[key]) < breadth(mine), (by_ref[key], mine)
