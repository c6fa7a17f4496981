"""The case database of the wide-grain assignment tests.  One 400-base segment; chunk A holds it under n_seq (TaxID, GI)
pairs, every sequence with BOTH orientations of it (so a read meets a (TaxID, GI) twice, at two offsets, on two strands),
TaxIDs and GIs with bit 31 set among them, a reverse palindrome (the same (TaxID, GI, offset) from both strands) and two
background sequences; chunk B repeats the even sequences with the same (TaxID, GI) and flanks but other substitutions (the
same long key with another edit) and gives the odd ones' TaxIDs a further GI.  census() counts what the tests require of
the oracle's hits before they look at the device."""
import random

import assign_cases
import helpers

SEED = 31
PALINDROME = (3000, 9000)
BACKGROUNDS = ((7, 1, 3000), (8, 2, 3000))


def tax_of(t):
    return (1000 + t // 3 if t < 30 else 1000 + t) | ((t & 1) << 31)


def gi_of(t):
    return (5000 + t) | (0xC0000000 if t % 3 == 0 else 0)


def _sequence(flanks, fwd, rev, fwd_first):
    a, b = (fwd, rev) if fwd_first else (rev, fwd)
    return flanks[0] + a + flanks[1] + b + flanks[2]


def database(n_seq=90, seed=SEED):
    """(entries of chunk A, entries of chunk B, seg, half, rng)"""
    rng = random.Random(seed)
    seg = helpers.rnd_seq(rng, 400)
    flanks = [[helpers.rnd_seq(rng, rng.randrange(60, 200)) for _ in range(3)] for _ in range(n_seq)]
    first = [(b[0], b[1], helpers.rnd_seq(rng, b[2])) for b in BACKGROUNDS]
    for t in range(n_seq):
        fwd = helpers.substitute(rng, seg, t % 4)
        rev = helpers.revcomp(helpers.substitute(rng, seg, 3 * t % 5))
        first.append((tax_of(t), gi_of(t), _sequence(flanks[t], fwd, rev, t % 2 == 0)))
    half = helpers.rnd_seq(rng, 200)
    first.append((*PALINDROME, helpers.rnd_seq(rng, 120) + half + helpers.revcomp(half) + helpers.rnd_seq(rng, 90)))
    second = []
    for t in range(n_seq):
        if t % 2 == 0:
            fwd = helpers.substitute(rng, seg, (t // 2) % 3)
            rev = helpers.revcomp(helpers.substitute(rng, seg, (t // 2 + 1) % 4))
            second.append((tax_of(t), gi_of(t), _sequence(flanks[t], fwd, rev, True)))
        else:
            second.append((tax_of(t), 7000 + t, flanks[t][0] + helpers.substitute(rng, seg, t % 3) + flanks[t][1]))
    return first, second, seg, half, rng


def reads(rng, seg, half, entries, n_seg=40, n_pal=10, n_bg=60):
    """windows of the segment with 0..3 edits, every other one reverse-complemented; reads across the palindrome's centre;
    ordinary reads of the backgrounds (one hit each)"""
    out = []
    for i in range(n_seg):
        st = rng.randrange(0, len(seg) - 150)
        r = helpers.mutate(rng, seg[st:st + 150], rng.randrange(0, 4), b"ACGT")
        out.append(helpers.revcomp(r) if i % 2 else r)
    pal = half + helpers.revcomp(half)
    for i in range(n_pal):
        st = 125 if i % 2 == 0 else 125 + rng.randrange(-40, 41)  # (centred: both strands give the same offset)
        out.append(helpers.mutate(rng, pal[st:st + 150], i % 3, b"ACGT"))
    out += assign_cases.background_reads(rng, entries[:len(BACKGROUNDS)], n_bg)
    return out


def census(hits):
    """what the hits of a batch hold, as a dict of counts:
    tax31 / gi31: reads whose records are ordered by a comparison of tax_id (of gi at equal tax_id) with bit 31 set on one side
    by_offset: (read, tax, gi) groups of more than one offset;  by_edit: long keys that occur with different edits
    edit_later: of those, the smaller edit not first;  same_edit: long keys that occur twice with equal edits
    winner_later: (read, tax, gi) groups whose smallest (edit, offset) is not their first hit
    offset_decides: groups whose two smallest hits have equal edits and different offsets
    group_max: the largest (read, tax, gi) group"""
    groups, keys, taxa, gis = {}, {}, {}, {}
    for r, t, g, o, e in zip(hits["read"].tolist(), hits["tax_id"].tolist(), hits["gi"].tolist(), hits["offset"].tolist(), hits["edit"].tolist()):
        groups.setdefault((r, t, g), []).append((e, o))
        keys.setdefault((r, t, g, o), []).append(e)
        taxa.setdefault(r, set()).add(t)
        gis.setdefault((r, t), set()).add(g)
    c = dict(tax31=0, gi31=0, by_offset=0, by_edit=0, edit_later=0, same_edit=0, winner_later=0, offset_decides=0, group_max=0, gis_max=0)
    c["tax31"] = sum(min(s) < 1 << 31 <= max(s) for s in taxa.values())
    c["gi31"] = sum(min(s) < 1 << 31 <= max(s) for s in gis.values())
    c["gis_max"] = max((len(s) for s in gis.values()), default=0)
    for v in groups.values():
        c["group_max"] = max(c["group_max"], len(v))
        c["by_offset"] += len({o for _, o in v}) > 1
        c["winner_later"] += min(v) != v[0]
        s = sorted(v)
        c["offset_decides"] += len(s) > 1 and s[0][0] == s[1][0] and s[0][1] != s[1][1]
    for es in keys.values():
        if len(es) > 1:
            if len(set(es)) > 1:
                c["by_edit"] += 1
                c["edit_later"] += min(es) != es[0]
            else:
                c["same_edit"] += 1
    return c
