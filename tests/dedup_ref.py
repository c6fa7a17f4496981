"""Plain-Python restatement of the dedup step (k_dedup.hip): which reads of a batch are identical, and the records of the
representatives fanned out to the reads they stand for.  No device, no library."""
import chain_ref as CR


def read_codes(bases, off):
    """the normalised codes of every read, as bytes"""
    codes = CR.normalise(bases)
    o = [int(x) for x in off]
    return [bytes(codes[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def rep(reads):
    """rep[j] = the smallest index whose read equals read j (reads: one bytes object of codes per read)"""
    first = {}
    return [first.setdefault(r, j) for j, r in enumerate(reads)]


def dupmap(reads, src_map=None):
    """(read, rep) in the caller's numbers: src_map[j] is the caller's number of resident read j (default: j)"""
    r = rep(reads)
    m = list(range(len(reads))) if src_map is None else [int(x) for x in src_map]
    return m, [m[k] for k in r]


def representatives(reads):
    return [j for j, k in enumerate(rep(reads)) if j == k]


def expand(records, read, rep_of):
    """records: tuples whose first field is the read, ordered by key; every entry (read[j], rep_of[j]) takes the records of
    rep_of[j] under the number read[j]"""
    by_read = {}
    for t in records:
        by_read.setdefault(t[0], []).append(t)
    return [(r,) + t[1:] for r, k in zip(read, rep_of) for t in by_read.get(k, [])]
