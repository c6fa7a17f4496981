"""The cases of test_consensus_cpu.py and test_consensus.py, on top of place_cases and pile_cases: a strain -- a mutated copy of
a stretch of one crafted reference, with reads that tile it -- and count tables for mtsv_pileup_add_counts on a small database
whose references meet at chosen lanes of a 64-slot tile.  Expected values are cons_ref's."""
import random

import helpers
import pile_cases as PL
import place_cases as PC
import place_ref as R

STRAIN_KEY = (2, 21)
STRAIN_LO, STRAIN_HI = 1800, 2400
STRAIN_SEED = 3
STRAIN_DEPTH = 3


def strain(entries, key=STRAIN_KEY, lo=STRAIN_LO, hi=STRAIN_HI, n_snps=5, seed=STRAIN_SEED):
    """a mutated copy of seq[lo:hi] of reference `key`: n_snps SNPs, none adjacent to another, a one-base deletion at a
    pile_cases.distinct_neighbours position and a one-base insertion elsewhere, all at least 40 bases apart and from the ends;
    reads of 60 to 100 bases of it from both strands, at least STRAIN_DEPTH over every base, as crafted hits.  Returns a dict:
    reads, hits ((read, tax_id, gi, offset, edit, strand)), snps {pos: base}, dele, ins (the reference position the extra base
    stands in front of), expected (the stretch as the consensus should spell it: SNPs and deletion applied, no insertion)"""
    rng = random.Random(seed)
    seq = PL.seq_of(entries)[key]
    assert 0 < lo < hi < len(seq) and b"N" not in seq[lo - 8:hi + 8]
    sites = list(range(lo + 40, hi - 48, 40))
    rng.shuffle(sites)
    assert len(sites) >= n_snps + 2
    snps = {p: rng.choice([b for b in b"ACGT" if b != seq[p]]) for p in sites[:n_snps]}
    dele = PL.distinct_neighbours(seq, sites[n_snps], sites[n_snps] + 8)
    ins = sites[n_snps + 1]
    ins_base = next(b for b in b"ACGT" if b != seq[ins - 1] and b != seq[ins])
    # the strain, and for each of its bases the reference position it stands on (the inserted base: the one behind it)
    bases, at = bytearray(), []
    for p in range(lo, hi):
        if p == ins:
            bases.append(ins_base)
            at.append(p)
        if p == dele:
            continue
        bases.append(snps.get(p, seq[p]))
        at.append(p)
    bases = bytes(bases)
    n = len(bases)
    starts = [0] * STRAIN_DEPTH + list(range(6, n - 60, 6))
    spans = [(s, min(s + rng.randrange(60, 101), n)) for s in starts] + [(n - rng.randrange(60, 101), n) for _ in range(STRAIN_DEPTH)]
    reads, hits = [], []
    for k, (s, e) in enumerate(spans):
        P = bases[s:e]
        assert 60 <= len(P) <= 100
        strand = k % 2
        offset = max(at[s] - 3, 0)
        edit = R.min_edit(R.codes(P), R.codes(seq[offset:at[e - 1] + 9]))
        reads.append(helpers.revcomp(P) if strand else P)
        hits.append((len(reads) - 1, key[0], key[1], offset, edit, strand))
    expected = "".join(chr(snps.get(p, seq[p])) for p in range(lo, hi) if p != dele)
    return dict(reads=reads, hits=hits, snps=snps, dele=dele, ins=ins, expected=expected, key=key, lo=lo, hi=hi)


# ---- count tables ----

# (tax_id, gi, L): L + 1 slots.  In key order the references begin at slots 0, 63, 127, 192, 321, 331 of their segment: the second
# begins in the last lane of a 64-slot tile, the fourth ends (slot 320) in the first lane of one, the fifth is shorter than a
# wavefront and lies between two long ones
SMALL_REFS = ((1, 10, 62), (1, 11, 63), (2, 20, 64), (2, 21, 128), (3, 30, 9), (3, 31, 299))
SMALL_READ_KEY, SMALL_READ_AT, SMALL_READ_LEN = (3, 31), 100, 40
ADD_HITS = 1000                                              # the n_hits of every add_counts call: no count above it


def small_database(seed=23):
    rng = random.Random(seed)
    entries = []
    for t, g, L in SMALL_REFS:
        s = bytearray(helpers.rnd_seq(rng, L))
        if L > 20:
            s[7:8] = b"N"                                    # a reference N
        entries.append((t, g, bytes(s)))
    offs, at = [], 0
    for _, _, L in SMALL_REFS:
        offs.append(at)
        at += L + 1
    assert offs == [0, 63, 127, 192, 321, 331] and offs[1] % 64 == 63 and (offs[3] + 128) % 64 == 0
    return entries


def small_read(entries):
    """(reads, hits): one clean read, so that an add_run teaches the accumulator the database's references"""
    seq = PL.seq_of(entries)[SMALL_READ_KEY]
    P = seq[SMALL_READ_AT:SMALL_READ_AT + SMALL_READ_LEN]
    return [P], [(0, SMALL_READ_KEY[0], SMALL_READ_KEY[1], SMALL_READ_AT, 0, 0)]


def random_slot(rng, last):
    """counters of every kind, none above ADD_HITS; last: a slot L takes insertions only"""
    n = [0] * 8
    kind = rng.randrange(10)
    if rng.randrange(3) == 0:
        n[7] = rng.choice([1, 2, 5, 40, ADD_HITS])
    if last or kind == 0:
        return n                                             # no depth
    if kind <= 3:
        n[0] = rng.randrange(1, 60)                          # a match majority with some noise
        n[rng.randrange(1, 7)] = rng.randrange(0, 4)
    elif kind <= 5:
        n[rng.randrange(1, 5)] = rng.randrange(2, 40)        # a substitution
        n[0] = rng.randrange(0, 3)
    elif kind == 6:
        n[6] = rng.randrange(1, 30)                          # a deletion
        n[0] = rng.randrange(0, 2)
    elif kind == 7:
        n[5] = rng.randrange(1, 9)                           # a read N
        n[rng.randrange(0, 5)] = rng.randrange(0, 9)
    else:
        for c in range(7):                                   # anything, ties among it
            n[c] = rng.randrange(0, 3)
    return n


def random_tables(entries, seed=31):
    """{key: [L + 1][8]} for every reference but (3, 30), which is deleted at every position"""
    rng = random.Random(seed)
    out = {}
    for t, g, s in entries:
        L = len(s)
        if (t, g) == (3, 30):
            out[(t, g)] = [[0, 0, 0, 0, 0, 0, 4, 0] for _ in range(L)] + [[0] * 8]
        else:
            out[(t, g)] = [random_slot(rng, p == L) for p in range(L + 1)]
    return out


# position -> counters, for a reference of at least 32 bases; what each is for stands beside it (min_depth 2 or 3,
# min_frac_ppm 500000 unless said otherwise)
EDGE_SLOTS = {
    0: [3, 3, 0, 0, 0, 0, 0, 0],          # match = A: match wins
    1: [0, 4, 0, 0, 4, 0, 0, 0],          # A = T: A wins
    2: [0, 0, 0, 0, 5, 0, 5, 0],          # T = del: T wins
    3: [2, 1, 1, 0, 0, 0, 0, 0],          # the winner exactly at half of depth 4: called
    4: [499, 251, 250, 0, 0, 0, 0, 0],    # one count below half of depth 1000: ambiguous
    5: [500, 250, 250, 0, 0, 0, 0, 0],    # exactly half: called
    6: [1, 0, 1, 0, 0, 3, 0, 0],          # a read-N majority: ambiguous
    7: [2, 0, 0, 0, 0, 0, 1, 0],          # depth 3: at min_depth 3, one below min_depth 4
    8: [1, 0, 0, 0, 0, 0, 1, 0],          # depth 2
    9: [1, 0, 0, 0, 0, 0, 0, 0],          # depth 1: covered at min_depth 0 and 1 alike
    10: [4, 0, 0, 0, 0, 0, 0, 2],         # 2 * ins == depth: no INS SITE
    11: [3, 0, 1, 0, 0, 0, 0, 3],         # 2 * ins == depth + 2 ...
    12: [4, 0, 1, 0, 0, 0, 0, 3],         # 2 * ins == depth + 1: an INS SITE
    13: [0, 0, 0, 0, 0, 0, 6, 0],         # a deletion
    14: [0, 0, 0, 0, 0, 0, 0, 5],         # insertions and no depth
    15: [0, 0, 7, 0, 0, 0, 0, 0],         # a clean substitution
}


def edge_table(L, ins_at_slot_l=3):
    assert L >= 32
    slots = [list(EDGE_SLOTS.get(p, [0] * 8)) for p in range(L)] + [[0] * 8]
    slots[L][7] = ins_at_slot_l
    return slots


def add_tables(table, more):
    """table += more, slot by slot"""
    for key, slots in more.items():
        for mine, n in zip(table[key], slots):
            for c in range(8):
                mine[c] += n[c]
