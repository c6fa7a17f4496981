"""The case databases of the deep-read tests (test_deep_reads_cpu.py, test_deep_reads.py): reads that carry thousands of
hits once up to 64 small chunk databases, each binned on its own, are merged.  Built on grain_cases.py: the same tax_of and
gi_of, so TaxIDs and GIs with bit 31 set are among the keys.

One fixed 400-base segment SEG (from a seed of its own, not a per-chunk one).  full_chunk(c) holds S_FULL sequences; sequence t
is flank + sub(SEG, a) + flank + revcomp(sub(SEG, b)) + flank under (tax_of(t), gi_of(t)), with 0..4 substitutions and flanks
of 60..199 bases drawn per (c, t).  A strand of a read returns a TaxID once, so the hits of a read of the segment in one
chunk are two per distinct TaxID: S_FULL = 74 sequences carry 64 distinct TaxIDs and give H = 128 hits per deep read and
chunk (64 sequences would carry 54 TaxIDs).  The same (TaxID, GI) recurs in every chunk and the offsets differ between
chunks; for even t the chunks 2p and 2p + 1 share their flanks and differ in their substitutions: the same long key with two
edits.  unit_chunk() is one sequence with one orientation of SEG[:250]: +1 hit for the deep reads whose window lies inside
it ("in"), +0 for the others ("out"), so one merge holds reads at E and at E + 1.  wide_chunk() is one database of S_WIDE
sequences (270 distinct TaxIDs): more than 512 hits of a deep read in a single run, on both strands.

Every case runs at the default parameters: none of max_hits, tune_max_hits, max_candidates, max_assignments cuts a list here
(test_deep_reads_cpu.py asserts the counts that show it).  The oracle's word on every chunk is computed once per process and
never changed."""
import random

import numpy as np

import assign_cases
import chunk_merge_ref as CM
import grain_cases as G
import helpers

SEG_SEED = 4243
S_FULL = 74
S_WIDE = 280
H = 128                     # hits of a deep read in one full chunk (asserted on the oracle's hits)
N_FULL = 64                 # the source limit of mtsv_batch_merge_runs
UNIT = (77777, 4242)        # (TaxID, GI) of the unit chunk's sequence
BACKGROUNDS = ((7, 1, 3000), (8, 2, 3000))
N_DEEP, N_BG, N_NONE = 24, 150, 30
IN_STARTS, OUT_STARTS = (0, 96), (165, 251)   # window starts inside SEG[:250] / with at most 85 bases inside it

_rng = random.Random(SEG_SEED)
SEG = helpers.rnd_seq(_rng, 400)
BG_ENTRIES = [(t, g, helpers.rnd_seq(_rng, n)) for t, g, n in BACKGROUNDS]


def _flanks(c, t):
    owner = f"pair{c // 2}" if t % 2 == 0 else f"chunk{c}"     # even t: chunks 2p and 2p + 1 share their flanks
    rng = random.Random(f"deep/flanks/{owner}/{t}")
    return [helpers.rnd_seq(rng, rng.randrange(60, 200)) for _ in range(3)]


def _sequence(c, t):
    rng = random.Random(f"deep/subs/{c}/{t}")
    fl = _flanks(c, t)
    fwd = helpers.substitute(rng, SEG, (t + c) % 5)
    rev = helpers.revcomp(helpers.substitute(rng, SEG, (3 * t + 2 * c + 1) % 5))
    return fl[0] + fwd + fl[1] + rev + fl[2]


def full_chunk(c, s=S_FULL):
    """entries (tax_id, gi, sequence) of full chunk c; chunk 0 also holds the two background sequences"""
    return (BG_ENTRIES if c == 0 else []) + [(G.tax_of(t), G.gi_of(t), _sequence(c, t)) for t in range(s)]


def unit_chunk():
    rng = random.Random("deep/unit")
    return [(*UNIT, helpers.rnd_seq(rng, 90) + SEG[:250] + helpers.rnd_seq(rng, 120))]


def wide_chunk(s=S_WIDE):
    return BG_ENTRIES + [(G.tax_of(t), G.gi_of(t), _sequence(1000, t)) for t in range(s)]


def reads():
    """(reads, kinds): N_DEEP windows of SEG with 0..3 edits, every other one reverse-complemented, alternately "in" and
    "out" of the unit chunk; N_BG reads of the backgrounds ("bg": one hit); N_NONE random reads ("none"); shuffled"""
    rng = random.Random(SEG_SEED + 1)
    out = []
    for i in range(N_DEEP):
        kind = "in" if (i // 2) % 2 == 0 else "out"
        st = rng.randrange(*(IN_STARTS if kind == "in" else OUT_STARTS))
        r = helpers.mutate(rng, SEG[st:st + 150], rng.randrange(0, 4), b"ACGT")
        out.append((helpers.revcomp(r) if i % 2 else r, kind))
    out += [(r, "bg") for r in assign_cases.background_reads(rng, BG_ENTRIES, N_BG)]
    out += [(helpers.rnd_seq(rng, 150), "none") for _ in range(N_NONE)]
    random.Random(SEG_SEED + 2).shuffle(out)
    return [r for r, _ in out], [k for _, k in out]


READS, KINDS = reads()
DEEP = [i for i, k in enumerate(KINDS) if k in ("in", "out")]
# two deep reads in one group of 64 reads (a ballot with more than one bit set) and two in different groups
assert len({i // 64 for i in DEEP}) > 1 and len({i // 64 for i in DEEP}) < len(DEEP)

# case -> (full chunks, with the unit chunk, MTSV_COLLAPSE_LDS_MAX or None); "one_pass" is wide_chunk() alone, no merge
CASES = {
    "two_trips": (5, False, None),
    "wide_edge": (16, True, None),
    "taxid_edge": (32, True, None),
    "ragged": (40, False, None),
    "full_house": (64, False, None),
    "moved_edge": (8, False, 1024),
    "one_pass": (0, False, None),
}


def chunk_keys(case):
    """the sources of a case, in merge order: ("full", c), ("unit",), ("wide",)"""
    if case == "one_pass":
        return [("wide",)]
    full, unit, _ = CASES[case]
    return [("full", c) for c in range(full)] + ([("unit",)] if unit else [])


def want_counts(case):
    """the hits a deep read of each kind must carry in the case: {"in": n, "out": n}; None where the oracle alone says"""
    if case == "one_pass":
        return None
    full, unit, _ = CASES[case]
    return {"in": full * H + int(unit), "out": full * H}


def entries_of(key):
    return full_chunk(key[1]) if key[0] == "full" else unit_chunk() if key[0] == "unit" else wide_chunk()


_parts, _merged = {}, {}


def batch():
    return helpers.reads_to_batch(READS)


def oracle_part(key):
    """the oracle's hits of READS on one chunk, at the default parameters (cached; about half a second a full chunk, one
    chunk at a time: the oracle's own threads take the reads of a chunk between them)"""
    if key not in _parts:
        from oracle import oracle as O
        bases, off = batch()
        _parts[key] = O.Index.build(entries_of(key)).bin_batch(bases, off, O.default_params(), threads=16)[0]
    return _parts[key]


def parts(case):
    return [oracle_part(k) for k in chunk_keys(case)]


def merged(case):
    """chunk_merge_ref.merge_hits of the case's parts (cached)"""
    if case not in _merged:
        _merged[case] = CM.merge_hits(parts(case))
    return _merged[case]


def per_read(hits):
    return np.bincount(hits["read"].astype(np.int64), minlength=len(READS))


def strand_counts(hits, read):
    s = hits["strand"][hits["read"] == read]
    return int((s == 0).sum()), int((s != 0).sum())
