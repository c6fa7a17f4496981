"""The database and reads of the assignment tests' tier cases: one 400-base segment planted under 90 TaxIDs with 0..6
substitutions, and again reverse-complemented under every third of them, so that a read of the segment carries about 120
hits on 90 distinct TaxIDs -- (read, TaxID) pairs that occur on both strands with different and with equal edits, the
smaller edit first or second."""
import random

import helpers

BACKGROUNDS = ((7, 1, 3000), (8, 2, 3000), (9, 3, 3000))


def tier_plants(rng, seg):
    """planted_db's plants: (segment, [(tax_id, gi)])"""
    first = [(helpers.substitute(rng, seg, 2 * (t % 4)), [(1000 + t, 5000 + t)]) for t in range(90)]
    second = [(helpers.revcomp(helpers.substitute(rng, seg, t % 5)), [(1000 + t, 7000 + t)]) for t in range(0, 90, 3)]
    return first, second


def tier_db(split=False):
    """(entries, seg, rng) -- split: (entries of the first chunk, of the second, seg, rng), the reverse-complemented plants
    in the second"""
    rng = random.Random(23)
    seg = helpers.rnd_seq(rng, 400)
    first, second = tier_plants(rng, seg)
    bg = list(BACKGROUNDS)
    if split:
        return helpers.planted_db(rng, bg[:2], first), helpers.planted_db(rng, bg[2:], second), seg, rng
    return helpers.planted_db(rng, bg, first + second), seg, rng


def tier_reads(rng, seg, n):
    reads = []
    for i in range(n):
        st = rng.randrange(0, len(seg) - 150)
        r = helpers.mutate(rng, seg[st:st + 150], rng.randrange(0, 5), b"ACGT")
        reads.append(helpers.revcomp(r) if i % 2 else r)
    return reads


def background_reads(rng, entries, n):
    """ordinary reads of the database's sequences, one or two hits each"""
    texts = [e[2].upper() for e in entries if len(e[2]) > 400]
    reads = []
    for i in range(n):
        t = rng.choice(texts)
        st = rng.randrange(0, len(t) - 150)
        r = helpers.mutate(rng, t[st:st + 150], rng.randrange(0, 3), b"ACGT")
        reads.append(helpers.revcomp(r) if i % 3 == 0 else r)
    return reads


def duplicate_census(hits):
    """of the (read, TaxID) pairs that occur twice: (different edits, of those the smaller edit second, equal edits)"""
    seen = {}
    for r, t, e in zip(hits["read"].tolist(), hits["tax_id"].tolist(), hits["edit"].tolist()):
        seen.setdefault((r, t), []).append(e)
    diff = later = same = 0
    for es in seen.values():
        if len(es) < 2:
            continue
        if es[0] == es[1]:
            same += 1
        else:
            diff += 1
            later += es[1] < es[0]
    return diff, later, same


def wave_db():
    """(entries, seg, rng): the same construction on 45 TaxIDs, so that a read of the segment carries 33..64 hits -- the
    wavefront tier with more than 32 lanes holding a key"""
    rng = random.Random(29)
    seg = helpers.rnd_seq(rng, 400)
    first = [(helpers.substitute(rng, seg, 2 * (t % 4)), [(2000 + t, 5000 + t)]) for t in range(45)]
    second = [(helpers.revcomp(helpers.substitute(rng, seg, t % 5)), [(2000 + t, 7000 + t)]) for t in range(0, 45, 3)]
    return helpers.planted_db(rng, list(BACKGROUNDS), first + second), seg, rng
