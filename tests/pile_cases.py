"""The cases of test_pile_cpu.py and test_pile.py, on top of place_cases: the same database (BIN_LEN = 4200, so 4201 slots
straddle every tile size) and crafted hits, second and third hits of a dozen reads, a deep pile with a planted SNP, deletion
and insertion, a read that reaches slot L, and a second database as a second chunk.  Expected values are pile_ref's."""
import random

import helpers
import pile_ref as PR
import place_cases as PC
import place_ref as R

DEEP_KEY = (2, 20)
DEEP_AT, DEEP_LEN, DEEP_READ = 1500, 200, 120          # the stretch every read of the deep pile is cut from, and their length
DEEP_SNP, DEEP_DEL = DEEP_AT + 88, DEEP_AT + 92       # inside every read with the insertion behind them: reads start in DEEP_AT .. DEEP_AT + 80
DEEP_N = {"clean": 550, "snp": 300, "del": 100, "ins": 50}
SLOT_L_KEY = (2, 21)
SLOT_L_READ = 90


def second_chunk():
    return PC.database(seed=6, first_tax=10)


def seq_of(*chunks):
    return {(t, g): s for entries in chunks for t, g, s in entries}


class Placer:
    """place_ref.place_hit with a memory: the expected (start, end, ops) of hits, equal hits computed once"""

    def __init__(self, *chunks):
        self.seq = seq_of(*chunks)
        self.seen = {}

    def __call__(self, reads, hits):
        out = []
        for r, t, g, o, e, strand in hits:
            key = (bytes(reads[r]), t, g, o, e, strand)
            if key not in self.seen:
                self.seen[key] = R.place_hit(reads[r], strand, self.seq[(t, g)], o, e)
            out.append(self.seen[key])
        assert all(p is not None for p in out)
        return out


def with_more_hits(reads, hits, n=12):
    """the crafted hits, and for n reads of 31 bases or more a second and a third hit on the same window at edit + 1 and
    edit + 2: placeable by the definition of `end`, the smallest column within the edit"""
    more, picked = list(hits), 0
    for k in range(0, len(hits), 7):
        r, t, g, o, e, strand = hits[k]
        if len(reads[r]) < 31 or picked == n:
            continue
        more += [(r, t, g, o, e + 1, strand), (r, t, g, o, e + 2, strand)]
        picked += 1
    assert picked == n
    return more


def distinct_neighbours(seq, lo, hi):
    """a position in lo .. hi - 1 whose base differs from both its neighbours, so a one-base deletion there aligns in one way"""
    for p in range(lo, hi):
        if seq[p] != seq[p - 1] and seq[p] != seq[p + 1]:
            return p
    raise AssertionError("no such position")


def deep_pile(entries, seed=41):
    """(reads, hits, planted): 1000 hits of reads of DEEP_READ bases cut from one stretch of 200 bases; exactly 300 carry a
    SNP at planted['snp'] (the read base planted['snp_base']), 100 lack the base at planted['del'], 50 carry an extra base in
    front of planted['ins'].  Both strands."""
    rng = random.Random(seed)
    seq = seq_of(entries)[DEEP_KEY]
    snp = DEEP_SNP
    dele = distinct_neighbours(seq, DEEP_DEL, DEEP_DEL + 8)
    ins = dele + 5
    snp_base = next(b for b in b"ACGT" if b != seq[snp])
    ins_base = next(b for b in b"ACGT" if b != seq[ins - 1] and b != seq[ins])
    reads, hits, made = [], [], {}
    for kind, count in DEEP_N.items():
        for k in range(count):
            start = DEEP_AT + rng.randrange(0, DEEP_LEN - DEEP_READ + 1)
            strand = rng.randrange(2)
            if (kind, start, strand) not in made:
                if kind == "clean":
                    P = seq[start:start + DEEP_READ]
                elif kind == "snp":
                    P = seq[start:snp] + bytes([snp_base]) + seq[snp + 1:start + DEEP_READ]
                elif kind == "del":
                    P = seq[start:dele] + seq[dele + 1:start + DEEP_READ + 1]
                else:
                    P = seq[start:ins] + bytes([ins_base]) + seq[ins:start + DEEP_READ - 1]
                assert len(P) == DEEP_READ
                offset = start - 3
                edit = R.min_edit(R.codes(P), R.codes(seq[offset:start + DEEP_READ + 8]))
                assert edit == (0 if kind == "clean" else 1)
                reads.append(helpers.revcomp(P) if strand else P)
                made[(kind, start, strand)] = (len(reads) - 1, DEEP_KEY[0], DEEP_KEY[1], offset, edit, strand)
            hits.append(made[(kind, start, strand)])
    rng.shuffle(hits)
    return reads, hits, {"snp": snp, "snp_base": "ACGT".index(chr(snp_base)), "del": dele, "ins": ins}


def slot_l_read(entries, seed=43):
    """(read, hit): the bin's last SLOT_L_READ - 1 bases and one base more that is not the bin's last, placed at the bin's end"""
    seq = seq_of(entries)[SLOT_L_KEY]
    extra = next(b for b in b"ACGT" if b != seq[-1])
    P = seq[len(seq) - (SLOT_L_READ - 1):] + bytes([extra])
    offset = len(seq) - (SLOT_L_READ - 1) - 2
    edit = R.min_edit(R.codes(P), R.codes(seq[offset:]))
    assert edit == 1
    return P, (0, SLOT_L_KEY[0], SLOT_L_KEY[1], offset, edit, 0)


def snp_reads(chunks, n=60, seed=47):
    """reads for the command line: cut from the chunks' sequences, 100 to 150 bases; those of the first chunk's second bin that
    cover position 2000 carry a planted SNP there in three of four; (reads, ids, (key, pos))"""
    rng = random.Random(seed)
    reads, ids = [], []
    key = (chunks[0][1][0], chunks[0][1][1])
    target = chunks[0][1][2]
    other = bytes([next(b for b in b"ACGT" if b != target[2000])])
    for k in range(n):
        L = rng.randrange(100, 151)
        if k % 2 == 0:
            start = 2000 - rng.randrange(10, L - 10)
            r = bytearray(target[start:start + L])
            if k % 8 != 0:
                r[2000 - start:2001 - start] = other
            r = bytes(r)
        else:
            seq = rng.choice([s for entries in chunks for _, _, s in entries])
            start = rng.randrange(0, len(seq) - 200)
            r = helpers.mutate(rng, seq[start:start + L], rng.randrange(0, 4), b"ACGT")
        reads.append(helpers.revcomp(r) if k % 3 == 0 else r)
        ids.append(f"read{k}")
    return reads, ids, (key, 2000)
