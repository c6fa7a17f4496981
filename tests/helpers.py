"""Shared generators for the test-suite: adversarial databases and read sets that reach the
order-dependent corners of the reference's hot loop (duplicate TaxIds, tie-breaking in the stable
rank sort, merged windows, seed thinning, bin-boundary clipping, N handling)."""
import hashlib
import random

import numpy as np

FIELDS = ("read", "tax_id", "gi", "edit", "strand", "offset")
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def rnd_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def mutate(rng, s, n_edits, alpha=b"ACGTN"):
    s = bytearray(s)
    for _ in range(n_edits):
        if not s:
            break
        op = rng.randrange(3)
        i = rng.randrange(len(s))
        if op == 0:
            s[i] = rng.choice(alpha)
        elif op == 1:
            del s[i]
        else:
            s.insert(i, rng.choice(b"ACGT"))
    return bytes(s)


def revcomp(s):
    return bytes(COMP.get(c, 78) for c in reversed(s.upper()))


def tricky_db(seed=7):
    """Returns (entries, gene, unit): entries = (tax, gi, seq) in database (file) order, gene = the
    conserved segment planted in many taxa, unit = the tandem-repeat unit."""
    rng = random.Random(seed)
    gene = rnd_seq(rng, 700)          # conserved gene present in many taxa / GIs
    unit = rnd_seq(rng, 97)           # tandem repeat unit
    entries = []
    gi = 1000
    taxa = [9, 2, 77, 40, 5, 123456, 31, 8, 4000000000, 17, 64, 3]
    for ti, tax in enumerate(taxa):
        for g in range(3):
            body = bytearray(rnd_seq(rng, rng.randrange(1500, 3000)))
            if ti < 8:  # conserved gene with 0..4 % divergence, several GIs per taxon
                at = rng.randrange(100, len(body) - 800)
                body[at:at + 700] = mutate(rng, gene, rng.randrange(0, 28), b"ACGT")[:700].ljust(700, b"A")
            if ti == 1 and g == 0:  # long tandem repeat: every seed hits ~40 sites, windows merge
                at = 50
                body[at:at + 97 * 40] = unit * 40
            if g == 1:  # runs of N and soft-masked / IUPAC bytes (index.rs:543-553)
                p = rng.randrange(0, len(body) - 200)
                body[p:p + rng.randrange(20, 120)] = b"N" * rng.randrange(20, 120)
                q = rng.randrange(0, len(body) - 60)
                body[q:q + 40] = bytes(body[q:q + 40]).lower()
                body[rng.randrange(len(body))] = ord("R")
            entries.append((tax, gi, bytes(body)))
            gi += rng.randrange(1, 50)
    # very short and empty sequences, same TaxId twice in different places of the file
    entries.append((2, 5, rnd_seq(rng, 40)))
    entries.append((2, 6, b""))
    entries.append((9, 7, rnd_seq(rng, 160)))
    entries.append((1, 8, rnd_seq(rng, 19)))
    rng.shuffle(entries)
    return entries, gene, unit


def ssw_live_pairs():
    """seeded (read, window) pairs of lengths 40..320 (the word kernel from 254 on), a third of them with N's: the
    inputs of tests/golden/ssw_live_golden.json"""
    rng = random.Random(99)
    pairs = []
    for L in (40, 100, 150, 253, 254, 320):
        for it in range(60):
            w = rnd_seq(rng, L + rng.randrange(0, 70), b"ACGTN" if it % 3 == 0 else b"ACGT")
            st = rng.randrange(0, max(1, len(w) - L + 1))
            read = mutate(rng, w[st:st + L], rng.randrange(0, L // 4)) if it % 2 else rnd_seq(rng, L)
            if len(read) < 30:
                continue
            pairs.append((read, w))
    return pairs


def pairs_digest(pairs):
    h = hashlib.sha256()
    for read, w in pairs:
        h.update(read + b"|" + w + b"\n")
    return h.hexdigest()


def reads_to_batch(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if reads else np.zeros(0, np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return bases, off


def tricky_reads(entries, gene, unit, seed=11, n_each=60, lengths=(150,)):
    """Reads aimed at the corners: conserved gene (many TaxIds / duplicate TaxIds), tandem repeat
    (hundreds of seed hits, merged windows), plain sequence with 0..ED+5 edits, reverse strand,
    N-rich, lower case / junk bytes, bin-boundary spanning, too short for a seed, empty."""
    rng = random.Random(seed)
    text_by_entry = [e[2].upper() for e in entries]
    long_entries = [t for t in text_by_entry if len(t) > 400]
    reads = []
    for L in lengths:
        for _ in range(n_each):  # conserved gene
            st = rng.randrange(0, len(gene) - L) if len(gene) > L else 0
            r = mutate(rng, gene[st:st + L], rng.randrange(0, 26))
            reads.append(r if rng.random() < 0.5 else revcomp(r))
        for _ in range(n_each // 2):  # tandem repeat
            rep = unit * 5
            st = rng.randrange(0, len(rep) - L) if len(rep) > L else 0
            reads.append(mutate(rng, rep[st:st + L], rng.randrange(0, 12)))
        for _ in range(n_each):  # ordinary reads with edit counts around the tolerance
            t = rng.choice(long_entries)
            st = rng.randrange(0, len(t) - L)
            r = mutate(rng, t[st:st + L], rng.choice([0, 1, 3, 8, 15, 19, 20, 21, 25, 40]))
            if rng.random() < 0.5:
                r = revcomp(r)
            if rng.random() < 0.2:
                r = r.lower()
            if rng.random() < 0.1:
                r = bytes(c if rng.random() > 0.05 else rng.choice(b"nRYK-*.") for c in r)
            reads.append(r)
        for _ in range(n_each // 3):  # spanning the junction of two database sequences
            a, b = rng.sample(long_entries, 2)
            k = rng.randrange(20, L - 20)
            reads.append(a[len(a) - k:] + b[:L - k])
    reads += [b"", b"A", b"ACGTACGTACGTACGTA", b"ACGTACGTACGTACGTAC", b"ACGTACGTACGTACGTACG",
              b"N" * 60, b"NNNNNNNNNNNNNNNNNN" + gene[:100], gene[:120] + b"N" * 30,
              rnd_seq(rng, 253), gene[:253], gene[100:130]]
    rng.shuffle(reads)
    return reads


def assert_same_hits(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], want[bad[:5]])


def substitute(rng, s, k, lo=0, hi=None, alpha=b"ACGT"):
    """k substitutions at distinct positions of s[lo:hi], each to a different base"""
    s = bytearray(s)
    hi = len(s) if hi is None else hi
    for i in rng.sample(range(lo, hi), min(k, max(0, hi - lo))):
        s[i] = rng.choice([c for c in alpha if c != s[i]] or alpha)
    return bytes(s)


def damage_at_end(rng, src, length, n_edits, span):
    """a read of `length` bases from src (which holds at least length + n_edits bases) with n_edits substitutions
    and indels, all in its last `span` bases: a candidate that fails does so in the last columns of its sweep"""
    r = bytearray(src[:length + n_edits])
    lo = max(0, length - span)
    for _ in range(n_edits):
        i = rng.randrange(lo, length)
        op = rng.randrange(3)
        if op == 0:
            r[i] = rng.choice([c for c in b"ACGT" if c != r[i]])
        elif op == 1:
            del r[i]
        else:
            r.insert(i, rng.choice(b"ACGT"))
    return bytes(r[:length])


def ladder_reads(rng, texts, L, edit_rate=0.13, n=240):
    """n reads whose longest is exactly L bases, the others spread over L/3..L, on both strands: exact copies,
    substitutions only, indels, ED-1 / ED / ED+1 edits (ED = ceil(len * edit_rate)), damage in the last bases,
    exactly ED and ED+1 N, reads cut at the start or end of a database sequence (clipped windows) and, from 254
    bases on, indels at the stripe rows k * ceil(L / 8) of the word kernel.  texts: database sequences, upper case."""
    import math
    long_texts = [t for t in texts if len(t) >= L + 40]
    reads = []
    for i in range(n):
        Lr = L if i % 4 == 0 else rng.randrange(max(1, L // 3), L + 1)
        ed = math.ceil(Lr * edit_rate)
        t = rng.choice(long_texts)
        st = rng.randrange(0, len(t) - Lr - 20)
        seg = t[st:st + Lr + 20]
        kind = i % 9
        if kind == 0:
            r = seg[:Lr]
        elif kind == 1:
            r = substitute(rng, seg[:Lr], rng.randrange(0, ed + 3))
        elif kind == 2:
            r = bytearray(seg)
            for _ in range(rng.randrange(1, min(8, ed + 1) + 1)):
                j = rng.randrange(Lr)
                if rng.random() < 0.5:
                    r[j:j] = rnd_seq(rng, rng.randrange(1, 3))
                else:
                    del r[j:j + rng.randrange(1, 3)]
            r = bytes(r[:Lr])
        elif kind == 3:
            r = substitute(rng, seg[:Lr], max(0, ed + (i // 9) % 3 - 1))
        elif kind == 4:
            r = damage_at_end(rng, seg, Lr, ed + (i // 9) % 2, ed + 4)
        elif kind == 5:
            r = bytes(c if c in b"ACGT" else 65 for c in seg[:Lr])   # no N but the planted ones
            r = substitute(rng, r, ed + (i // 9) % 2, alpha=b"N")
        elif kind == 6:
            t = rng.choice(long_texts)
            r = t[:Lr] if (i // 9) % 2 else t[len(t) - Lr:]
            r = substitute(rng, r, rng.randrange(0, ed + 1))
        elif kind == 7 and L >= 254:
            seg8 = (L + 7) // 8
            r = bytearray(seg)
            for _ in range(rng.randrange(1, 4)):
                b = rng.randrange(1, 8) * seg8 + rng.randrange(-2, 3)
                k = rng.randrange(1, 5)
                if rng.random() < 0.6:
                    r[b:b] = rnd_seq(rng, k)
                else:
                    del r[b:b + k]
            r = bytes(r[:Lr])
        else:
            r = mutate(rng, seg[:Lr], rng.randrange(0, ed + 2), b"ACGT")[:Lr]
        reads.append(r if rng.random() < 0.5 else revcomp(r))
    assert max(map(len, reads)) == L
    return reads


def planted_db(rng, background, plants):
    """A database of random sequences with segments planted a known number of times.
    background: [(tax_id, gi, length)] random sequences; plants: [(segment, [(tax_id, gi), ...])] -- one exact copy of
    the segment in a sequence of its own (random flanks of 60..200 bases) for every listed (tax_id, gi).
    Returns the entries (tax_id, gi, sequence) in that order."""
    entries = [(tax, gi, rnd_seq(rng, n)) for tax, gi, n in background]
    for seg, owners in plants:
        for tax, gi in owners:
            entries.append((tax, gi, rnd_seq(rng, rng.randrange(60, 200)) + seg + rnd_seq(rng, rng.randrange(60, 200))))
    return entries
