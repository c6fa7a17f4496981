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


# ---- the index geometry ladder (test_index_geometry_cpu.py, test_index_geometry.py) ----------------------------------
# One rung = one database whose text (the concatenation of its sequences plus '$') has exactly n symbols, with its own
# sampling intervals.  The kinds and sizes sit where the device index and the GPU builder branch on n, on the row of
# the sentinel, on the suffix sampling interval or on the composition of the text.

RANDOM_N = (1, 2, 3, 17, 18, 19, 25, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769,
            65535, 65536, 65537, 131071, 131072, 131073, 524159, 524160, 524161)
# (n = 1, the text "$" of one empty sequence, leads the tiny rungs: 2 and 3 hold one and two bases; 17, 18, 19 end one
# short of, at, and one past the first text that holds a default seed of 18 symbols; 25 holds one probe of 24)
SENTINEL_N = 4096
SENTINEL_TARGETS = ("res0", "res1", "res63", "res64", "res127", "first_block", "last_block")
SENTINEL_TRIES = 4096
SAMPLING_N = (4097, 257)
REPEAT_KINDS = ("A", "AC", "tandem97")


def sampling_intervals(n):
    return [(k, s) for s in (1, 2, 3, 7, 31, 32, n - 1, n, n + 1, 1 << 20) for k in (1, 64, n + 5)]


def _fast_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choices(alpha, k=n)) if n else b""


def _cut_into_bins(rng, body, n_cuts=4):
    """body in a handful of sequences of uneven length with one empty sequence among them; TaxIDs ascend with the order
    (so the order of the entries is the order of the text), two of them twice"""
    L = len(body)
    cuts = sorted(rng.randrange(0, L + 1) for _ in range(n_cuts if L else 0))
    edges = [0] + cuts + [L]
    seqs = [body[a:b] for a, b in zip(edges, edges[1:])]
    seqs.insert(min(2, len(seqs)), b"")
    taxa = (2, 2, 5, 9, 9, 4000000000, 4000000001)
    return [(taxa[i], 100 + 7 * i, s) for i, s in enumerate(seqs)]


def geometry_db(kind, n, rng):
    """entries (tax_id, gi, sequence), already in the order of the text, whose sequences hold n - 1 symbols in all"""
    L = n - 1
    if kind == "random":
        entries = _cut_into_bins(rng, _fast_seq(rng, L))
    elif kind == "sentinel":  # random text with a few N runs of 1..30 symbols
        body = bytearray(_fast_seq(rng, L))
        for _ in range(rng.randrange(3, 7)):
            k = rng.randrange(1, 31)
            at = rng.randrange(0, L - k)
            body[at:at + k] = b"N" * k
        entries = _cut_into_bins(rng, bytes(body))
    elif kind == "A":
        entries = _cut_into_bins(rng, b"A" * L)
    elif kind == "AC":
        entries = _cut_into_bins(rng, (b"AC" * (L // 2 + 1))[:L])
    elif kind == "tandem97":
        unit = _fast_seq(rng, 97)
        entries = _cut_into_bins(rng, (unit * (L // 97 + 1))[:L])
    elif kind == "nrun":  # one run of 5000 N in random text
        body = bytearray(_fast_seq(rng, L))
        at = rng.randrange(100, L - 5100)
        body[at:at + 5000] = b"N" * 5000
        entries = _cut_into_bins(rng, bytes(body))
    elif kind == "ACG":
        entries = _cut_into_bins(rng, _fast_seq(rng, L, b"ACG"))
    elif kind == "CGT":
        entries = _cut_into_bins(rng, _fast_seq(rng, L, b"CGT"))
    elif kind == "tinybins":  # 6000 sequences of 0..39 symbols over 2000 taxa
        lens = [rng.randrange(0, 40) for _ in range(6000)]
        while sum(lens) != L:
            i = rng.randrange(6000)
            d = 1 if sum(lens) < L else -1
            if 0 <= lens[i] + d < 40:
                lens[i] += d
        taxa = sorted(rng.randrange(1, 2001) for _ in range(6000))
        entries = [(taxa[i], 10 + i, _fast_seq(rng, k)) for i, k in enumerate(lens)]
    else:
        raise ValueError(kind)
    assert sum(len(e[2]) for e in entries) + 1 == n, (kind, n)
    return entries


def geometry_text(entries):
    return b"".join(e[2] for e in entries)


_sentinel_seeds = None


def sentinel_seeds():
    """{target: (seed, row)} of the sentinel-row rungs: the first seeds whose database puts the row of the whole text (the
    row whose BWT symbol is '$') at each residue modulo 128, and into the first and the last rank block.  The row comes
    from the oracle: lo of backward_search(text[:40]) when that interval has one row.  Residue 0 is where the derived
    rank of N changes its meaning (the sentinel lies "before the block" from the next block on), and a block shows its
    rank of N only where one of its rows holds an N in the BWT: that rung also wants the suffix behind one of its N runs
    in the sentinel row's block, which a probe with one N in front of that suffix then finds."""
    global _sentinel_seeds
    if _sentinel_seeds is None:
        import re
        from oracle import oracle as O
        n = SENTINEL_N
        found = {}
        for seed in range(SENTINEL_TRIES):
            if len(found) == len(SENTINEL_TARGETS):
                break
            entries = geometry_db("sentinel", n, random.Random(0x5E17 * 4096 + seed))
            text = geometry_text(entries)
            ix = O.Index.build(entries, 64, 32)
            ok, lo, hi = ix.backward_search(text[:40])
            if not ok or hi - lo != 1:
                continue
            hit = ["res%d" % (lo % 128)]
            if lo < 128:
                hit.append("first_block")
            if lo >= ((n - 1) >> 7) << 7:
                hit.append("last_block")
            if lo % 128 == 0:
                behind = [ix.backward_search(text[m.end():m.end() + 40]) for m in re.finditer(rb"N+", text)]
                if not any(ok2 and h2 - l2 == 1 and lo <= l2 < lo + 128 for ok2, l2, h2 in behind):
                    hit.remove("res0")
            for t in hit:
                if t in SENTINEL_TARGETS:
                    found.setdefault(t, (seed, lo))
        assert len(found) == len(SENTINEL_TARGETS), sorted(set(SENTINEL_TARGETS) - set(found))
        _sentinel_seeds = found
    return _sentinel_seeds


class Rung:
    def __init__(self, name, kind, n, occ_k=64, sa_s=32, target=None):
        self.name, self.kind, self.n, self.occ_k, self.sa_s, self.target = name, kind, n, occ_k, sa_s, target

    def __repr__(self):
        return self.name

    def entries(self):
        if self.kind == "sentinel":
            seed = 0x5E17 * 4096 + sentinel_seeds()[self.target][0]
        else:
            seed = int.from_bytes(hashlib.sha256(("%s/%d" % (self.kind, self.n)).encode()).digest()[:6], "big")
        return geometry_db(self.kind, self.n, random.Random(seed))

    def sentinel_row(self):
        return sentinel_seeds()[self.target][1]


def _rungs():
    out = [Rung("random-%d" % n, "random", n) for n in RANDOM_N]
    out += [Rung("sentinel-%s" % t, "sentinel", SENTINEL_N, target=t) for t in SENTINEL_TARGETS]
    out += [Rung("A-65536", "A", 65536), Rung("AC-65536", "AC", 65536), Rung("tandem97-20000", "tandem97", 20000),
            Rung("A-3000", "A", 3000), Rung("AC-3000", "AC", 3000), Rung("tandem97-3000", "tandem97", 3000),
            Rung("A-129", "A", 129, occ_k=3, sa_s=5),
            Rung("nrun-20000", "nrun", 20000), Rung("ACG-65536", "ACG", 65536), Rung("CGT-32768", "CGT", 32768),
            Rung("ACG-4096", "ACG", 4096, occ_k=128, sa_s=7),
            Rung("tinybins-117001", "tinybins", 117001)]
    for n in SAMPLING_N:
        out += [Rung("sampling-%d-k%d-s%d" % (n, k, s), "random", n, occ_k=k, sa_s=s) for k, s in sampling_intervals(n)]
    return out


RUNGS = _rungs()
RUNG_BY_NAME = {r.name: r for r in RUNGS}
assert len(RUNG_BY_NAME) == len(RUNGS)


def kmer_width_for(n):
    """the k-mer table width the upload picks for a text of n symbols (dev_index.hip), where HBM is no limit"""
    k = 1
    while k < 16 and 4 ** (k + 1) <= 2 * n:
        k += 1
    return 17 if k == 16 and n >= 1 << 31 else k


def position_probes(text, exhaustive_up_to=131073, width=24):
    """[(text position, read)]: every substring of `width` symbols of the text (of the whole text, where it is shorter),
    alternately as it stands and reverse-complemented; on texts of more than exhaustive_up_to symbols every 5th position
    and the first and last 300"""
    L = len(text)
    w = min(width, L)
    if w == 0:
        return []
    last = L - w
    if L + 1 <= exhaustive_up_to:
        pos = range(0, last + 1)
    else:
        pos = sorted(set(range(0, last + 1, 5)) | set(range(0, 300)) | set(range(last - 299, last + 1)))
    return [(i, text[i:i + w] if k % 2 == 0 else revcomp(text[i:i + w])) for k, i in enumerate(pos)]


def n_edge_probes(rng, text):
    """reads of 30..60 symbols across both edges of every N run of the text, placed so that their first seed of 18
    symbols holds 1..18 N, on both strands"""
    L = len(text)
    runs, i = [], 0
    while i < L:
        if text[i] == 78:
            j = i
            while j < L and text[j] == 78:
                j += 1
            runs.append((i, j))
            i = j
        else:
            i += 1
    reads = []
    for a, b in runs:
        for k in range(1, 19):
            for start in (a - (18 - k), b - k):
                start = max(0, min(start, L - 30))
                r = text[start:start + rng.randrange(30, 61)]
                reads.append(r if len(reads) % 2 == 0 else revcomp(r))
    return reads


def geometry_reads(rng, entries, n=300):
    """n ordinary reads of 40..150 symbols: ladder_reads where a sequence is long enough for it, else damaged pieces of
    the text (which then span the junctions of its short sequences)"""
    import math
    texts = [e[2] for e in entries]
    if any(len(t) >= 190 for t in texts):
        return ladder_reads(rng, texts, 150, n=n)
    text = b"".join(texts)
    reads = []
    for _ in range(n):
        Lr = rng.randrange(40, min(150, len(text)) + 1)
        st = rng.randrange(0, len(text) - Lr + 1)
        r = mutate(rng, text[st:st + Lr], rng.randrange(0, math.ceil(Lr * 0.13) + 3))
        reads.append(r if rng.random() < 0.5 else revcomp(r))
    return reads


# ---- chains of refused candidates (test_verify_rounds_cpu.py, test_verify_rounds.py) ---------------------------------
# One chain = one TaxID whose sequences (one GI each, in file order, between random flanks of 80..200 bases) are damaged
# copies of one random segment.  All damage lies inside one region [lo, hi] of the segment, every copy changes lo and hi,
# and every 18-mer that touches the region holds a change in every copy: a read cut across the region keeps the same
# intact seeds on all of them, they tie in the rank order, and the stable sort leaves them in file order.  With
# ED = ceil(0.13 * L) and thr = L - 2 * ED, D the unit-cost distance under the SW matrix's matches:
#   A  every region base complemented                              D > 2*ED: the bound refutes it
#   B  nB substitutions lo..hi, ED < nB <= 2*ED, L - 2*nB < thr     undecided by the bound, the sweep refutes it
#   C  s substitutions + i bases inserted at hi - 4,               undecided, the score passes (i + 2*s <= 2*ED), the edit
#      ED < s + i <= 2*ED                                          distance s + i refuses it
#   G  nG <= ED substitutions lo..hi                               accepted
# and for reads that hold N at 180..191 of the segment (region 180..239, L = 150):
#   g  5 substitutions                                             accepted with 17 edits
#   e  N under the read's N + 13 substitutions                     D = 13 <= ED < 25 edits: passes the bound, refused
#   b  17 substitutions, bases under the read's N                  D = 29: undecided, the sweep refutes it
#   c  N under the read's N + the 5 of g + 16 bases inserted       D = 21: undecided, the score passes, 33 edits refuse it
CHAIN_LO = 180
CHAIN_SHAPES = {  # L: region length, nG, nB, C's (s, i), read starts lo - (first .. last)
    150: dict(region=90, nG=9, nB=26, s=9, i=14, back=(15, 35)),
    96: dict(region=50, nG=5, nB=14, s=5, i=10, back=(19, 24)),
    253: dict(region=160, nG=15, nB=34, s=15, i=20, back=(20, 50)),
}
CHAIN_N_SHAPE = dict(region=60, back=(15, 35))  # the N family: L = 150, read starts 145..165


def _spread(lo, hi, n):
    """n positions evenly spaced from lo to hi, both included"""
    return sorted({lo + round(k * (hi - lo) / (n - 1)) for k in range(n)}) if n > 1 else [lo]


def _complemented(seg, positions):
    s = bytearray(seg)
    for p in positions:
        s[p] = COMP[s[p]]
    return s


def chain_copy(rng, seg, kind, L):
    """the copy of `kind` of a segment whose region starts at CHAIN_LO"""
    lo = CHAIN_LO
    if kind in "ABCG":
        sh = CHAIN_SHAPES[L]
        hi = lo + sh["region"] - 1
        if kind == "A":
            return bytes(_complemented(seg, range(lo, hi + 1)))
        if kind == "B":
            return bytes(_complemented(seg, _spread(lo, hi, sh["nB"])))
        if kind == "G":
            return bytes(_complemented(seg, _spread(lo, hi, sh["nG"])))
        s = _complemented(seg, _spread(lo, hi - 12, sh["s"] - 1) + [hi])
        s[hi - 4:hi - 4] = rnd_seq(rng, sh["i"])
        return bytes(s)
    assert L == 150
    if kind == "g":
        return bytes(_complemented(seg, [192, 204, 216, 228, 239]))
    if kind == "b":
        return bytes(_complemented(seg, list(range(192, 240, 3)) + [239]))
    if kind == "e":
        s = _complemented(seg, list(range(192, 240, 4)) + [239])
        s[180:192] = b"N" * 12
        return bytes(s)
    if kind == "c":
        s = _complemented(seg, [192, 204, 216, 228, 239])
        s[180:192] = b"N" * 12
        s[235:235] = rnd_seq(rng, 16)
        return bytes(s)
    raise ValueError(kind)


def chain_kinds(with_n=False):
    """the chains of one database: every sequence over the three failing kinds of length 1..3, once ending in a good copy
    and once without one; for the reads without N also CCCC, CCCCC and CCCCCC before a good copy (seven copies: a cut at
    max_candidates = 6 falls inside a chain too)"""
    import itertools
    fail, good = ("ebc", "g") if with_n else ("ABC", "G")
    out = []
    for n in (1, 2, 3):
        for t in itertools.product(fail, repeat=n):
            out += ["".join(t) + good, "".join(t)]
    if not with_n:
        out += ["CCCCG", "CCCCCG", "CCCCCCG"]
    return out


class ChainDb:
    """entries: (tax_id, gi, sequence) in file order; chains: [(tax_id, kinds, [gi per copy])]; segments: the segment of
    every chain; copies: {gi: the copy between its flanks}; reads: the batch, with read_chain[k] the index into chains of
    read k"""

    def __init__(self, L, entries, chains, segments, copies, reads, read_chain):
        self.L, self.entries, self.chains, self.segments, self.copies = L, entries, chains, segments, copies
        self.reads, self.read_chain = reads, read_chain

    def kinds_of(self, k):
        return self.chains[self.read_chain[k]][1]

    def good_gi(self, k):
        tax, kinds, gis = self.chains[self.read_chain[k]]
        return gis[-1] if kinds[-1] in "Gg" else None


def chain_db(rng, L, with_n=False, reads_per_strand=3):
    """the chain database for reads of L bases and its reads: reads_per_strand exact cuts of every chain's segment per
    strand (with N at 180..191 for the N family), in the order of the chains"""
    sh = CHAIN_N_SHAPE if with_n else CHAIN_SHAPES[L]
    seg_len = CHAIN_LO + sh["region"] + 180
    entries = [(10 + t, 500 + t, rnd_seq(rng, 3000)) for t in range(3)]
    chains, segments, copies, reads, read_chain = [], [], {}, [], []
    for ci, kinds in enumerate(chain_kinds(with_n)):
        seg = rnd_seq(rng, seg_len)
        tax = 1000 + ci
        gis = []
        for k, kind in enumerate(kinds):
            gi = 100000 + 10 * ci + k
            copies[gi] = chain_copy(rng, seg, kind, L)
            entries.append((tax, gi, rnd_seq(rng, rng.randrange(80, 201)) + copies[gi] + rnd_seq(rng, rng.randrange(80, 201))))
            gis.append(gi)
        chains.append((tax, kinds, gis))
        segments.append(seg)
        src = bytearray(seg)
        if with_n:
            src[180:192] = b"N" * 12
        for k in range(2 * reads_per_strand):
            st = CHAIN_LO - rng.randrange(sh["back"][0], sh["back"][1] + 1)
            r = bytes(src[st:st + L])
            reads.append(r if k < reads_per_strand else revcomp(r))
            read_chain.append(ci)
    return ChainDb(L, entries, chains, segments, copies, reads, read_chain)


def chain_prediction(kinds):
    """(prefilter runs, edit distances, hits) of the reference for a read of a chain: every copy up to the good one is
    prefiltered, the copies whose score passes (C, c, e and the good one) get an edit distance, the good one is the hit"""
    g = 1 if kinds[-1] in "Gg" else 0
    return len(kinds), sum(k in "Cce" for k in kinds) + g, g


def expected_rounds(kinds):
    """n_rounds of the default arrangement for a read of a chain (mtsv_amd.h, the mode comment of k_edit_myers).
    A lane of k_edit_myers (fused in round 0, list mode behind every sweep) refutes A and walks on, passes e, refuses it
    and walks on, accepts G/g; an undecided kind (B C b c) met in the fused lane goes to the sweep of the same round, met
    in a list lane it starts a new round.  The sweep fails A B b and walks on; what it passes (C c e, G g) goes to a list
    lane, which refuses C c e and walks on, and accepts G g.  n_rounds = 1 + the times a list lane met an undecided kind."""
    rounds, where = 1, "fused"
    for k in kinds:
        if where == "sweep":
            if k in "ABb":
                continue
            if k in "Gg":
                break
            where = "list"  # C c e: passed by the sweep, refused by the list lane, which walks on
            continue
        if k == "A" or k == "e":
            continue
        if k in "Gg":
            break
        if where == "list":
            rounds += 1
        if k in "Cc":  # the sweep of this round passes it, its list lane refuses it and walks on
            where = "list"
        else:  # B b: the sweep refutes it and walks on
            where = "sweep"
    return rounds


CHAIN_CASES = ((96, False), (150, False), (253, False), (150, True))  # (L, the N family)
CHAIN_SEED = 4100
_chain_cases = {}


def chain_case(L, with_n=False):
    """the chain database of (L, family), built once per process, with the oracle's word on it: .orc the oracle's index
    of the entries, .per_read [(hits, counters)] of every read binned alone at default parameters, .as_predicted [bool]
    whether (n_sw, n_edit, hits) of read k is chain_prediction() of its chain"""
    key = (L, bool(with_n))
    if key not in _chain_cases:
        from concurrent.futures import ThreadPoolExecutor
        from oracle import oracle as O
        db = chain_db(random.Random(CHAIN_SEED), L, with_n)
        db.orc = O.Index.build(db.entries)
        op = O.default_params()

        def one(r):
            b, o = reads_to_batch([r])
            return db.orc.bin_batch(b, o, op, threads=1)

        with ThreadPoolExecutor(8) as ex:
            db.per_read = list(ex.map(one, db.reads))
        db.as_predicted = [(c["n_sw"], c["n_edit"], len(h)) == chain_prediction(db.kinds_of(k))
                           for k, (h, c) in enumerate(db.per_read)]
        _chain_cases[key] = db
    return _chain_cases[key]
