"""The crafted hits of test_place_cpu.py and test_place.py: a small database, reads cut from it with a planted edit script,
and for each a hit whose window begins a chosen number of columns before the planted match.  A hit's edit is what the binner
would give it -- the smallest last-row entry over a window that holds the planted match -- computed by place_ref; nothing
here comes from the device."""
import random

import numpy as np

import helpers
import place_ref as R

LENGTHS = (1, 31, 32, 33, 63, 64, 65, 128, 129, 160, 161, 224, 255, 256)      # every template width at its word edge
SCRIPTS = ("none", "x_first", "x_last", "i_first", "i_last", "d_first", "d_last", "mixed")
PLACES = ("at_start", "one_in", "far_in", "bin_end", "text_end", "text_begin")
FAR = 3000                                                                # columns before a far match: the ring wraps
BIN_LEN = 4200
N_AT = 3500                                                               # every bin holds an N here and at N_AT + 1


def database(seed=5, first_tax=1):
    """(tax_id, gi, seq) in index order: ascending TaxID, the first bin at text position 0, the last ending before '$'"""
    rng = random.Random(seed)
    entries = []
    for tax, gi in ((first_tax, 10), (first_tax + 1, 20), (first_tax + 1, 21), (first_tax + 2, 30)):
        body = bytearray(helpers.rnd_seq(rng, BIN_LEN))
        body[N_AT:N_AT + 2] = b"NN"
        entries.append((tax, gi, bytes(body)))
    return entries


def planted_read(rng, seg_of, L, script):
    """a read of L bases cut from seg_of(n) -- the n reference bases at the planted site -- with the script applied"""
    other = lambda c: rng.choice([b for b in b"ACGT" if b != c])
    if script in ("none", "x_first", "x_last"):
        r = bytearray(seg_of(L))
        if script == "x_first":
            r[0] = other(r[0])
        elif script == "x_last":
            r[-1] = other(r[-1])
        return bytes(r)
    if script in ("i_first", "i_last"):                       # a read base the reference does not have
        s = seg_of(L - 1)
        at = min(1, len(s)) if script == "i_first" else max(len(s) - 1, 0)
        return s[:at] + bytes([rng.choice(b"ACGT")]) + s[at:]
    if script in ("d_first", "d_last"):                       # a reference base the read does not have
        s = seg_of(L + 1)
        at = 1 if script == "d_first" else L - 1
        return (s[:at] + s[at + 1:])[:L] if L > 1 else s[:1]
    s = helpers.mutate(rng, seg_of(L + L // 2), int(0.45 * L), b"ACGT")
    return (s + helpers.rnd_seq(rng, L))[:L]


def ref_bases(script, L):
    """the reference bases the planted site of a script other than "mixed" takes"""
    if script.startswith("i_"):
        return L - 1
    if script.startswith("d_") and L > 1:
        return L + 1
    return L


def crafted(entries, seed=17):
    """(reads, hits): hits as (read, tax_id, gi, offset, edit, strand), one read each; every length x script x strand, the
    window places taking turns, and a read N over a text N per length"""
    rng = random.Random(seed)
    reads, hits = [], []
    text_of = {(t, g): s for t, g, s in entries}
    first, last = (entries[0][0], entries[0][1]), (entries[-1][0], entries[-1][1])
    middle = (entries[1][0], entries[1][1])
    turn = 0

    def add(key, site, delta, L, script, strand):
        seq = text_of[key]
        P = planted_read(rng, lambda n: seq[site:site + n], L, script)
        assert len(P) == L
        offset = site - delta
        window = R.codes(seq[offset:site + 2 * L + 2])
        edit = R.min_edit(R.codes(P), window)
        reads.append(helpers.revcomp(P) if strand else P)
        hits.append((len(reads) - 1, key[0], key[1], offset, edit, strand))

    for L in LENGTHS:
        for script in SCRIPTS:
            for strand in (0, 1):
                where = PLACES[turn % len(PLACES)]
                turn += 1
                if where == "at_start":
                    add(middle, 700 + turn, 0, L, script, strand)
                elif where == "one_in":
                    add(middle, 900 + turn, 1, L, script, strand)
                elif where == "far_in":
                    add(middle, FAR + 40 + turn, FAR, L, script, strand)
                elif where in ("bin_end", "text_end"):        # the planted site ends on the bin's last base
                    sc = "x_first" if script == "mixed" else script
                    add(middle if where == "bin_end" else last, BIN_LEN - ref_bases(sc, L), 5, L, sc, strand)
                else:
                    add(first, 0, 0, L, script, strand)
        for strand in (0, 1):                                 # the read keeps the reference's two N in its middle: an X each, never a match
            if L >= 4:
                add(middle, N_AT + 1 - L // 2, 3, L, "none", strand)
    return reads, hits


def hits_array(hits, dtype):
    a = np.zeros(len(hits), dtype=dtype)
    for k, name in enumerate(("read", "tax_id", "gi", "offset", "edit", "strand")):
        a[name] = [h[k] for h in hits]
    return a


def expected(entries, reads, hits):
    """place_ref's (ref_start, ref_end, ops) per hit"""
    text_of = {(t, g): s for t, g, s in entries}
    return [R.place_hit(reads[r], strand, text_of[(t, g)], o, e) for r, t, g, o, e, strand in hits]


def paired_reads(chunks, n_pairs=40, seed=29):
    """mates cut from the chunks' sequences, 100 to 150 bases, up to six edits, mate 2 from the other strand: (reads, ids)"""
    rng = random.Random(seed)
    seqs = [s for entries in chunks for _, _, s in entries]
    reads, ids = [], []
    for p in range(n_pairs):
        seq = rng.choice(seqs)
        at = rng.randrange(0, len(seq) - 500)
        for mate in (0, 1):
            L = rng.randrange(100, 151)
            start = at + mate * rng.randrange(100, 300)
            r = helpers.mutate(rng, seq[start:start + L], rng.randrange(0, 7), b"ACGT")
            reads.append(helpers.revcomp(r) if mate else r)
            ids.append(f"frag{p}/{mate + 1}")
    return reads, ids
