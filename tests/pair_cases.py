"""Record lists for mtsv_fold_pair (k_pair.hip): shared by test_pair_cpu.py and test_pair.py.

A case is (n_reads, records): `records` are wide tuples (read, tax_id, gi, offset, edit) in any order, reads 2p and 2p + 1 the
mates of pair p.  project() makes of them the list a fold of a grain would hold -- one record per key of the grain with the
better value, in key order (fold_ref) -- and that list is what both the library and pair_ref are given."""
import numpy as np

import fold_ref as F

GRAINS = {"taxid": F.TAXID, "taxid_gi": F.TAXID_GI, "long": F.LONG}
U32 = 2 ** 32 - 1
HIGH = 2 ** 31


def project(grain, wide):
    if grain == F.TAXID:
        return F.fold(grain, [(r, t, e) for r, t, _, _, e in wide], [])
    return F.fold(grain, wide, [])


def as_array(grain, recs, dtypes):
    """the records of project() as the structured array of the grain; dtypes = (ASSIGN_DTYPE, ASSIGN_GI_DTYPE)"""
    a = np.zeros(len(recs), dtype=dtypes[0] if grain == F.TAXID else dtypes[1])
    for k, r in enumerate(recs):
        a[k] = r
    return a


def edges():
    """16 reads: the first and the last pair, pairs without records, with records of one mate only, TaxIDs with bit 31 set, and
    taxa only mate 1 has below, between and above mate 0's"""
    recs = [(0, 5, 1, 10, 2), (0, 5, 1, 90, 1), (1, 5, 1, 50, 3),                       # the first pair
            # pair 1: no record
            (4, 3, 1, 0, 1), (4, HIGH + 1, 2, 7, 0),                                      # pair 2: mate 0 only
            (7, 9, 1, 5, 4), (7, 11, 1, 5, 0),                                            # pair 3: mate 1 only
            (8, 10, 1, 100, 1), (8, 20, 1, 100, 2),                                       # pair 4: mate 1's taxa around mate 0's
            (9, 5, 1, 100, 0), (9, 10, 1, 150, 3), (9, 15, 1, 100, 1), (9, 20, 2, 100, 0), (9, 25, 1, 100, 2),
            (10, HIGH, 3, 40, 1), (10, U32, HIGH, 40, 2), (11, HIGH, 3, 44, 5), (11, U32, HIGH, 30, 0), (11, U32 - 1, 1, 1, 1),
            # pair 6: no record
            (14, 7, 1, 1000, 0), (14, 7, 1, 2000, 1), (15, 7, 1, 2100, 2), (15, 8, 1, 0, 0)]  # the last pair
    return 16, recs


def offsets():
    """offsets 0 and 2^32 - 1: a window that wrapped would find the mate at the other end"""
    recs = [(0, 7, 1, 0, 1), (0, 7, 1, U32, 2), (1, 7, 1, 1, 1), (1, 7, 1, U32 - 1, 2),   # couples at distance 1 at both ends
            (2, 7, 1, U32, 0), (3, 7, 1, 0, 0),                                            # distance 2^32 - 1, mate 0 at the top
            (4, 7, 1, 0, 0), (5, 7, 1, U32, 0),                                            # ... and at the bottom
            (6, 7, 1, 0, 3), (7, 7, 1, 0, 4), (8, 7, 1, U32, 3), (9, 7, 1, U32, 4)]       # distance 0 at both ends
    return 10, recs


def windows(sizes=(1, 3, 4, 16, 17, 18)):
    """per size w two pairs whose mate 0 has one record and whose window in mate 1 holds exactly w records, by TaxID (records of
    one (tax_id, gi) at offsets 1000, 1001, ...) and, with max_insert 20, by offset (w records within 20 of mate 0's offset and
    one more on either side, 21 away); the smallest edit sits in the window's last record, then in its first"""
    recs, read = [], 0
    for w in sizes:
        for best in (w - 1, 0):
            recs.append((read, 50, 1, 2000, 1))
            recs.append((read, 60, 1, 2000, 0))
            for k in range(w):
                off = 2000 - 20 + (40 * k) // max(w - 1, 1) if w > 1 else 2000
                recs.append((read + 1, 50, 1, off, 2 if k == best else 5))
            recs.append((read + 1, 50, 1, 2000 - 21, 0))
            recs.append((read + 1, 50, 1, 2000 + 21, 0))
            recs.append((read + 1, 50, 2, 2000, 0))                                       # another GI: in BOTH, out of PROPER
            read += 2
    return read, recs


def straddle():
    """tile 64: a pair of about 200 records whose runs and mate boundary straddle tiles; record 63 of the LONG list, the last of
    its tile, is a run's head; ordinary pairs before and behind"""
    recs = [(0, 1, 1, k, 3 + k % 4) for k in range(63)]                                   # records 0 .. 62: one run
    recs += [(0, 2, 1, k, 9 - k % 7) for k in range(70)]                                  # its head is record 63
    recs += [(1, 1, 1, 30 + k, 1 + k % 3) for k in range(40)] + [(1, 2, 1, 500 + k, k % 5) for k in range(30)] + [(1, 3, 1, 0, 0)]
    for p in range(1, 30):
        recs += [(2 * p, 1 + p % 3, 1, 10 * p, p % 4), (2 * p + 1, 1 + p % 3, 1, 10 * p + p, p % 3), (2 * p + 1, 2 + p % 3, 1, 0, 1)]
    return 60, recs


def heavy(n=2048, others=40):
    """one pair with n records per mate in one (tax_id, gi), offsets one apart -- with max_insert 500 the windows run to about
    1000 records -- among ordinary pairs"""
    recs = []
    for p in range(others):
        recs += [(2 * p, 4, 1, 100 + p, p % 3), (2 * p + 1, 4, 1, 300 + p, p % 2), (2 * p + 1, 6, 1, 10, 0)]
    h = 2 * others
    recs += [(h, 4, 1, 10000 + k, 2 + (k * 7) % 11) for k in range(n)]
    recs += [(h + 1, 4, 1, 10400 + k, 1 + (k * 5) % 13) for k in range(n)]
    recs += [(h, 9, 1, 5, 0), (h + 1, 9, 1, 700, 0)]
    for p in range(others + 1, 2 * others):
        recs += [(2 * p, 4, 2, 100 + p, p % 3), (2 * p + 1, 4, 2, 90 + p, p % 2)]
    return 4 * others, recs


def random_pairs(rng, n_pairs=2000, longest=40, n_taxa=6, n_gis=3, max_off=3000, max_edit=6):
    recs = []
    for read in range(2 * n_pairs):
        if rng.random() < 0.15:
            continue
        k = rng.choice((1, 1, 2, 3, 5, rng.randrange(0, longest + 1)))
        seen = set()
        for _ in range(k):
            key = (10 + rng.randrange(n_taxa), 1 + rng.randrange(n_gis), rng.randrange(max_off + 1))
            if key not in seen:
                seen.add(key)
                recs.append((read, *key, rng.randrange(max_edit + 1)))
        # a mate 1 now and then sits on, or next to, a record of its mate 0: couples at distance 0 and 1
        if read & 1 and recs and recs[-1][0] >= read - 1 and rng.random() < 0.4:
            _, t, g, o, _ = rng.choice([r for r in recs[-2 * longest - 2:] if r[0] == read - 1] or [recs[-1]])
            key = (t, g, min(max(o + rng.choice((-1, 0, 0, 1)), 0), max_off))
            if key not in seen:
                recs.append((read, *key, rng.randrange(max_edit + 1)))
    return 2 * n_pairs, recs
