"""Cases built onto the structural edges of the tiled passes (k_lca, k_pair, k_abund, k_fold, k_text, k_parse), for every tile
size the code accepts: shared by test_tile_ladders_cpu.py, which asserts that the cases hold what they claim, and test_tile_ladders.py,
which runs them on the device.  Generators and coverage functions only: what a case must give comes from the restatements
(lca_ref, pair_ref, abund_ref, fold_ref, text_cases.text, parse_ref), never from here.

A stage runs 256 lanes over a tile of T items; a lane owns a STRETCH of s(T) = max(T / 256, 1) consecutive items (the
ceiling for fold and text) and a wavefront 64 * s(T).  A structural edge of kind E in {s, 64 * s, T} is a position that is a
multiple of E; a kind whose E is 1, or equals a smaller kind's, is skipped.  An event stands "at every side" of kind E when
it stands at E - 1, E and E + 1 -- the first edge of the kind -- and at m - 1, m and m + 1 for a multiple m of E behind the
first tile.  Two events cannot always stand next to each other (a token is several bytes, an equal pair two positions, a
read with an outlier at least two records), so a generator gives one list per side d: its events stand at m + d for every
edge m.  missing() is the coverage condition, computed by the coverage functions from the lists alone."""
import bisect
import functools
import random

import numpy as np

import fold_ref as F
import parse_cases as PC
import text_cases as TC

LANES = 256
SIDES = (-1, 0, 1)
LCA_TILES = (64, 128, 256, 512, 1024)
PAIR_TILES = (64, 128, 256, 512, 1024)
ABUND_TILES = (64, 128, 256, 512, 1024)
FOLD_TILES = (2, 64, 128, 256, 512, 1024)
TEXT_TILES = (2, 64, 128, 256, 512, 1024)
PARSE_TILES = (64, 256, 1024, 4096, 8192, 16384)
B31 = 1 << 31


def stretch(T, ceil=False):
    return max((T + LANES - 1) // LANES if ceil else T // LANES, 1)


def kinds(T, ceil=False):
    s, out = stretch(T, ceil), []
    for E in (s, 64 * s, T):
        if E > 1 and E not in out:
            out.append(E)
    return out


def edges(T, E, floor=0):
    """(the first edge of kind E, one behind the first tile); floor: the first edge is the first multiple of E not below it
    (the parser: a token start cannot stand at byte 3, 4 or 5 of a text whose tokens have seven bytes or more)"""
    first = E * max(1, -(-floor // E))
    return first, first + max(T, E)


def targets(T, d, ceil=False, floor=0):
    return sorted({m + d for E in kinds(T, ceil) for m in edges(T, E, floor)})


def missing(positions, T, ceil=False, floor=0, sides=SIDES):
    """the (E, side, which edge) at which no event of `positions` stands: empty when the events stand at every side of every kind"""
    out = []
    for E in kinds(T, ceil):
        first = edges(T, E, floor)[0]
        for d in sides:
            if first + d not in positions:
                out.append((E, d, "first"))
            if not any((p - d) % E == 0 and p - d > max(T, first) for p in positions):
                out.append((E, d, "later"))
    return out


# ---- LCA ----------------------------------------------------------------------------------------------------------------------
# The outlier taxonomy: root 1, its child 100, under 100 the children 50, 60 and 70.  The leaves are the TaxIDs 1000 .. 4749: one
# that ends in 3 hangs under 50 (375 low outliers), one that ends in 7 under 70 (375 high outliers), the other 3000 under 60 (the
# fillers).  Records inside a read are sorted by TaxID, so an outlier's TaxID decides where it stands in the read; preorder (children
# ascending by TaxID) numbers 50's subtree below every filler and 70's above.  A read of fillers and one low outlier has the LCA 100;
# losing that record's contribution to the segmented minimum of node numbers gives 60, and the high outlier does the same to the maximum.
LEAF_LO, LEAF_HI = 1000, 4750


def leaf_parent(t):
    return {3: 50, 7: 70}.get(t % 10, 60)


OUTLIER = ("1 | 1 | root\n100 | 1 | clade\n50 | 100 | low\n60 | 100 | mid\n70 | 100 | high\n" +
           "".join(f"{t} | {leaf_parent(t)} | leaf\n" for t in range(LEAF_LO, LEAF_HI)))
FILLERS = [t for t in range(LEAF_LO, LEAF_HI) if leaf_parent(t) == 60]
LOWS = [t for t in range(LEAF_LO, LEAF_HI) if leaf_parent(t) == 50]
HIGHS = [t for t in range(LEAF_LO, LEAF_HI) if leaf_parent(t) == 70]


def _taxa(rng, length, at=None, pool=None):
    """`length` ascending leaf TaxIDs: fillers next to each other, with one TaxID of `pool` at index `at`"""
    if pool is None:
        i = rng.randrange(0, len(FILLERS) - length + 1)
        return FILLERS[i:i + length]
    ok = [x for x in pool if at <= bisect.bisect(FILLERS, x) <= len(FILLERS) - (length - 1 - at)]
    x = rng.choice(ok)
    i = bisect.bisect(FILLERS, x)
    return FILLERS[i - at:i] + [x] + FILLERS[i:i + length - 1 - at]


def lca_read(rng, read, length, best, outlier=None):
    """the records of one read: index `best` holds its smallest edit, every other record one more; outlier: (index, pool)"""
    base = 1 + (5 * read) % 11
    taxa = _taxa(rng, length, *(outlier or (None, None)))
    return [(read, t, base if k == best else base + 1) for k, t in enumerate(taxa)]


def _lca_list(rng, n, heads, special):
    """(records, n_reads): n records, read heads at `heads` and at 0; special {position: 'b' | 'c' | 'd'}: the read's smallest
    edit, its low outlier, its high outlier.  A read without a 'b' gets its smallest edit at a record of its own choice."""
    heads = sorted(set(heads) | {0})
    recs, read = [], 0
    for a, b in zip(heads, heads[1:] + [n]):
        read += rng.randrange(1, 3)
        best = outlier = None
        for p, k in special.items():
            if a <= p < b:
                if k == "b":
                    assert best is None
                    best = p - a
                else:
                    assert outlier is None and b - a >= 2
                    outlier = (p - a, LOWS if k == "c" else HIGHS)
        if best is None:
            best = rng.choice([j for j in range(b - a) if not outlier or j != outlier[0]])
        recs += lca_read(rng, read, b - a, best, outlier)
    return recs, read + 2


def lca_span(T):
    return 64 * stretch(T)


@functools.lru_cache(maxsize=None)
def lca_cases(T):
    """{name: (records, n_reads)}: per side d the heads at every edge (heads), and the events b, c, d at every edge, each in
    a read of its own; three reads measured against one wavefront span (spans); a read longer than two tiles with its
    smallest edit in one of its tiles and an outlier in the next (long)"""
    rng = random.Random(9000 + T)
    out = {}
    for d in SIDES:
        tg = targets(T, d)
        n = max(200, tg[-1] + max(T // 2, 20))
        out[f"heads{d:+d}"] = _lca_list(rng, n, tg, {})
        between = [p + (q - p + 1) // 2 for p, q in zip(tg, tg[1:])]
        for k in "bcd":
            out[f"{k}{d:+d}"] = _lca_list(rng, n, between, {p: k for p in tg})
    S = lca_span(T)
    # [0, S - 1) fills span 0 but for its last record, [S, 2S) fills span 1, [2S + 1, 3S) span 2 but for its first record
    out["spans"] = _lca_list(rng, max(200, 3 * S + 20), [S - 1, S, 2 * S, 2 * S + 1, 3 * S, 3 * S + 9],
                             {S // 2: "b", S - 2: "c", 2 * S - 1: "b", S: "c", 2 * S + 1: "b", 3 * S - 1: "d"})
    first, length = 3, 2 * T + 40
    where = ((first + T) // 2, T + T // 2, 2 * T + 20)                            # a position in the read's first, middle and last tile
    for rot in range(3):
        for k in "cd":
            out[f"long{rot}{k}"] = _lca_list(rng, max(200, first + length + 4), [first, first + length], {where[rot]: "b", where[(rot + 1) % 3]: k})
    return out


def reads_of(recs):
    """[(first position, end)] of the reads of a sorted list"""
    out, i = [], 0
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j][0] == recs[i][0]:
            j += 1
        out.append((i, j))
        i = j
    return out


def lca_events(recs):
    """what stands where, from the records alone: {'heads', 'b', 'c', 'd'} -> positions"""
    ev = {"heads": set(), "b": set(), "c": set(), "d": set()}
    for i, j in reads_of(recs):
        ev["heads"].add(i)
        edits = [r[2] for r in recs[i:j]]
        par = [leaf_parent(r[1]) for r in recs[i:j]]
        m = min(edits)
        if j - i > 1 and edits.count(m) == 1 and all(e == m + 1 for e in edits if e != m) and par[edits.index(m)] == 60:
            ev["b"].add(i + edits.index(m))
        for pool, other, key in ((50, 70, "c"), (70, 50, "d")):
            if par.count(pool) == 1 and other not in par and 60 in par:
                ev[key].add(i + par.index(pool))
    return ev


# ---- runs: pairs and abundance ------------------------------------------------------------------------------------------------
# Wide records (read, tax_id, gi, offset, edit).  k_pair's segments are the RUNS of one (read, tax_id); k_abund counts read heads and
# run heads.  Reads count up by one, so reads 2p and 2p + 1 are the mates of a pair, and a read's TaxIDs begin at 1 or 2 and go up
# by 1 or 2, so mates share most of theirs.  Inside a run the key ascends by `vary`: "offset" (GI 1, the mates' records within
# reach of each other: a list for the LONG grain) or "gi" (a list for both wide grains).

def run_list(rng, n, run_heads, read_heads, vary="offset", edit=None, read0=0, tax5=range(0)):
    """(records, n_reads): n records, a new read at `read_heads` and at 0, a new run at `run_heads` as well; edit: {position: edit}
    for the records that do not get theirs by chance; read0: the first read; tax5: the positions (of whole reads of one run)
    whose TaxID is 5"""
    recs, read, tax, step = [], read0 - 1, 0, 0
    for p in range(n):
        if p == 0 or p in read_heads:
            read, tax, step = read + 1, 1 + rng.randrange(2), 0
        elif p in run_heads:
            tax, step = tax + rng.randrange(1, 3), 0
        else:
            step += rng.randrange(1, 4)
        t, e = 5 if p in tax5 else tax, (edit or {}).get(p, rng.randrange(6))
        recs.append((read, t, 1, step, e) if vary == "offset" else (read, t, 1 + step, 3, e))
    return recs, (read + 4) & ~1


def narrow(recs):
    """the (read, tax_id, edit) of wide records whose (read, tax_id) are distinct: the same list at the TAXID grain"""
    out = [(r[0], r[1], r[4]) for r in recs]
    assert len(set(r[:2] for r in out)) == len(out)
    return out


def run_heads_of(recs):
    """(read heads, run heads) of a sorted list, from the records alone"""
    reads = {p for p, r in enumerate(recs) if p == 0 or r[0] != recs[p - 1][0]}
    return reads, {p for p, r in enumerate(recs) if p == 0 or r[:2] != recs[p - 1][:2]}


@functools.lru_cache(maxsize=None)
def run_cases(T, vary="offset"):
    """{name: (records, n_reads)} per side d: the read heads at every edge and nowhere else, every record a run of its own
    (reads: narrow() makes the TAXID grain's list of it); the run heads at every edge and nowhere else, every second of them a
    read head (runs)"""
    rng = random.Random(8000 + T + (vary == "gi"))
    out = {}
    for d in SIDES:
        tg = targets(T, d)
        n = max(200, tg[-1] + max(T // 2, 20))
        out[f"reads{d:+d}"] = run_list(rng, n, set(range(n)), set(tg), vary)
        out[f"runs{d:+d}"] = run_list(rng, n, set(tg), set(tg[1::2]), vary)
    return out


# The headless tile, at tile 64: a segment [40, 200) begins inside tile 0 and ends inside tile 3, so tiles 1 and 2 hold no head,
# their only rank is 0 and one cell is the tile's first segment and its last at once.  Its smallest value is unique and stands
# in tile 1, in tile 2 or at the last record of tile 0.
HEADLESS_T, HEADLESS_SEG, HEADLESS_N = 64, (40, 200), 230
HEADLESS_AT = {"tile1": 100, "tile2": 150, "tile0_last": 63}


def headless_reads(at):
    """(records, n_reads) for k_lca, at the TAXID grain: the segment is a read of 160 TaxIDs, its smallest edit at `at` and a
    low outlier of the taxonomy OUTLIER in another tile without a head"""
    a, b = HEADLESS_SEG
    return _lca_list(random.Random(at), HEADLESS_N, [20, a, b, b + 12], {at: "b", 150 if at != 150 else 100: "c"})


def headless_runs(at, kernel):
    """(records, n_reads), wide.  kernel 'read': the segment is a read of 160 runs of one record, edits 3 but for a 1 at `at`.
    kernel 'pair': the segment is the one run of read 2, edits 3 but for a 1 at `at`; its mate, read 3, is the one record behind
    it, of the same TaxID and within 480 bases of every record of the run.  kernel 'abund': the segment is a run inside a read
    [30, 210) that has a run before it and one behind it; the run's smallest edit, 2, stands at `at`, the read's, 1, at 205 in
    tile 3, the other records have 4 (slack 1: the run enters by its smallest edit alone)"""
    a, b = HEADLESS_SEG
    rng = random.Random(at)
    if kernel == "read":    # every record a run of its own, the segment is read 2: narrow() makes the TAXID grain's list of it
        edit = {p: 3 for p in range(a, b)}
        edit[at] = 1
        return run_list(rng, HEADLESS_N, set(range(HEADLESS_N)), {20, a, b, b + 12}, "gi", edit)
    if kernel == "pair":
        edit = {p: 3 for p in range(a, b)}
        edit[at] = 1
        return run_list(rng, HEADLESS_N, {10, 20, 30, a, b, b + 1, b + 10, b + 20}, {20, a, b, b + 1, b + 20}, "offset", edit, tax5=range(a, b + 1))
    edit = {p: 4 for p in range(30, b + 10)}
    edit[at], edit[205] = 2, 1
    return run_list(rng, HEADLESS_N, {10, 20, 30, a, b, b + 10, b + 20}, {10, 30, b + 10}, "gi", edit)


# A whole tile of one-record segments, then a segment that begins at the tile's last position and goes on for nine records in
# the next tile, its smallest edit at T + 3: every position of the tile is a head (of both kinds), `total` is the tile, and the
# tile's last segment is a single record in it.
def full_tile_heads(T):
    return set(range(T)) | {T + 9, T + 12, T + 20}


def full_tile_reads(T):
    """(records, n_reads) for k_lca at the TAXID grain: the segments are reads; a low outlier at T + 6"""
    return _lca_list(random.Random(T), T + 30, sorted(full_tile_heads(T)), {T + 3: "b", T + 6: "c"})


def full_tile_runs(T, vary="offset", one_run=True):
    """(records, n_reads), wide.  one_run: the segment is the one run of read T, an even read, and its mate, read T + 1, is a
    run of the same TaxID behind it; otherwise every record is a run of its own (narrow() makes the TAXID grain's list of it)"""
    heads = full_tile_heads(T)
    edit = {p: 3 for p in range(T - 1, T + 9)}
    edit[T + 3] = 1
    return run_list(random.Random(T), T + 30, heads if one_run else set(range(T + 30)), heads, vary, edit, read0=1,
                    tax5=range(T - 1, T + 12) if one_run else range(0))


# ---- fold -----------------------------------------------------------------------------------------------------------------------

def fold_rec(grain, k, edit, offset=0):
    """the record of key number k (keys ascend with their number, 32 per read) with the given value; bit 31 set in some fields"""
    read, low = k >> 5, k & 31
    if grain == F.TAXID:
        return (read, low | (B31 if low >= 16 else 0), edit)
    if grain == F.TAXID_GI:
        return (read, low >> 2, (low & 3) | (B31 if low & 2 else 0), offset, edit)
    return (read, low >> 3, (low >> 2) & 1, (0, 1, 2, 0xFFFFFFFF)[low & 3], edit)   # LONG: the offset belongs to the key


def _fold_lists(grain, rng, layout):
    """(A, B) whose merged sequence (duplicates kept, A first among equals) is `layout`: 'A', 'B', or 'P' / 'p' for a B record whose
    key is that of the A record one position before.  The 'P' pairs in turn: B better, A better, B better, A better -- at TAXID_GI
    the last two by the offset alone, their edits equal; a 'p' pair is one of the four by chance."""
    a, b, key, n_pairs = [], [], -1, 0
    for p, what in enumerate(layout):
        if what not in "Pp":
            key += rng.randrange(1, 3)
            (a if what == "A" else b).append(fold_rec(grain, key, rng.randrange(0, 6), rng.randrange(0, 4)))
            continue
        assert layout[p - 1] == "A"
        phase = n_pairs % 4 if what == "P" else rng.randrange(4)
        n_pairs += what == "P"
        values = ((4, 1, 2, 3), (2, 3, 4, 1), (3, 7, 3, 2), (3, 2, 3, 7)) if grain == F.TAXID_GI else ((4, 0, 2, 0), (2, 0, 4, 0), (5, 0, 1, 0), (1, 0, 5, 0))
        ea, oa, eb, ob = values[phase]
        a[-1] = fold_rec(grain, key, ea, oa)
        b.append(fold_rec(grain, key, eb, ob))
    return a, b


@functools.lru_cache(maxsize=None)
def fold_cases(grain, T):
    """{name: (A, B)}: per side d the equal pairs whose B record stands at every edge (pairs); a tile of A records alone, one of B
    records alone, and a run of pairs, every second position dropped, over several stretches (blocks)"""
    rng = random.Random(7000 + 10 * T + grain)
    out = {}
    for d in SIDES:
        tg = targets(T, d, ceil=True)
        n = max(200, tg[-1] + max(T // 2, 20))
        layout = [rng.choice("AB") for _ in range(n)]
        keep = {q for p in tg for q in (p - 1, p)}
        for p in tg:
            layout[p - 1], layout[p] = "A", "P"
        for p in range(1, n):
            if p not in keep and layout[p - 1] == "A" and layout[p] == "B" and rng.random() < 0.3:
                layout[p] = "p"
        out[f"pairs{d:+d}"] = _fold_lists(grain, rng, layout)
    s = stretch(T, ceil=True)
    n = max(200, 3 * T)
    layout = ["A"] * T + ["B"] * T + [rng.choice("AB") for _ in range(n - 2 * T)]
    at = 2 * T + s + 1
    for i in range(2 * s + 2):
        layout[at + 2 * i], layout[at + 2 * i + 1] = "A", "P"
    out["blocks"] = _fold_lists(grain, rng, layout)
    return out


def fold_layout(grain, a, b):
    """from the lists alone: (which list every merged position comes from, {position of a pair's B record: 'A' | 'B', the list
    that holds the better value, '=' when the values are equal})"""
    seq = sorted([(F.split(grain, r), 0) for r in a] + [(F.split(grain, r), 1) for r in b], key=lambda x: (x[0][0], x[1]))
    which = "".join("AB"[w] for _, w in seq)
    pairs = {}
    for p in range(1, len(seq)):
        (ka, va), wa = seq[p - 1]
        (kb, vb), wb = seq[p]
        if ka == kb:
            assert (wa, wb) == (0, 1)
            pairs[p] = "B" if vb < va else "A" if va < vb else "="
    return which, pairs


# ---- text -----------------------------------------------------------------------------------------------------------------------

def text_cap(T):
    return min(max(32 * T, 256), 32768)


def item_len(grain, r):
    return len(f"{r[1]}={r[2]}") if grain == F.TAXID else len(f"{r[1]}-{r[2]}-{r[3]}={r[4]}")


def _text_heads(grain, rng, T, d):
    tg = set(targets(T, d, ceil=True))
    near = {q + e for dd in SIDES for q in targets(T, dd, ceil=True) for e in (-2, -1, 0, 1, 2)}
    n = max(200, max(tg) + max(T // 2, 20))
    records, read, k = [], 0, 0
    for p in range(n):
        if p == 0 or p in tg or (p not in near and rng.random() < 0.4):
            read += rng.randrange(1, 3)
            k = 0
        records.append(TC.rec(grain, read, 10 * k + rng.randrange(10), rng.randrange(1000), rng.randrange(100000), rng.randrange(12)))
        k += 1
    return TC.finish(grain, rng, records, [rng.randrange(21) for _ in range(read + 2)])


def _text_residues(grain, rng, T=1024, tiles=17):
    """`tiles` full tiles and a few records more; the text of every full tile is one byte more than a multiple of 16, so the k-th
    tile edge of the output is k modulo 16"""
    c = TC.spread(grain, rng, tiles * T + 10, max_id=12)
    lengths = [len(s) for s in c.ids]
    for t in range(tiles):
        tile = range(t * T, (t + 1) * T)
        head = next(p for p in tile if c.records[p][0] != c.records[p - 1][0])       # (p >= 1: a tile of 1024 records holds a head behind its first)
        total = sum(item_len(grain, c.records[p]) + 1 + (lengths[c.records[p][0]] + 1 if p == 0 or c.records[p][0] != c.records[p - 1][0] else 0)
                    for p in tile)
        lengths[c.records[head][0]] += (1 - total) % 16
    return TC.finish(grain, rng, c.records, lengths)


WINDOW_KINDS = ("two_caps", "short_id", "long_id", "digits", "separator")


def _text_windows(grain, rng, T):
    """one tile per kind of WINDOW_KINDS.  Every such tile begins with a read of one record whose ID is as long as it takes to
    put the tile's second record where the kind wants it, measured from the first window edge W of the tile: the first
    multiple of 16 not above the tile's first byte, and cap(T) more"""
    cap = text_cap(T)
    records, lengths, at, read = [], {}, 0, 0

    def push(new_read, id_len, tax, edit):
        nonlocal at, read
        if new_read:
            read += 1
            lengths[read] = id_len
            at += id_len + 1
        r = TC.rec(grain, read, tax, 7, 3, edit)
        records.append(r)
        at += item_len(grain, r) + 1

    for kind in WINDOW_KINDS:
        while len(records) % T:
            push(True, rng.randrange(1, 9), rng.randrange(100), rng.randrange(10))
        W = (at & ~15) + cap
        i0 = item_len(grain, TC.rec(grain, 0, 5, 7, 3, 1))
        before = {"two_caps": None, "short_id": 20, "long_id": 50, "digits": 5, "separator": 0}[kind]  # W minus the second record's first byte
        pad = 2 * cap + 50 if before is None else W - before - at - i0 - 2
        push(True, pad, 5, 1)
        assert before is None or at == W - before
        if kind == "digits":
            push(False, 0, 1234567890, 4)
        else:
            push(True, {"short_id": 40, "long_id": 100}.get(kind, 6), 77, 2)
    for _ in range(3):
        push(True, 4, 9, 9)
    return TC.finish(grain, rng, records, [lengths.get(i, 0) for i in range(read + 2)])


@functools.lru_cache(maxsize=None)
def text_cases(grain, T):
    """the cases of text_cases.cases, and: read heads at every edge per side d, the windows, and at 1024 the residues"""
    rng = random.Random(6000 + 10 * T + grain)
    out = dict(TC.cases(grain))
    for d in SIDES:
        out[f"heads{d:+d}"] = _text_heads(grain, rng, T, d)
    out["windows"] = _text_windows(grain, rng, T)
    if T == 1024:
        out["residues"] = _text_residues(grain, rng)
    return out


def text_heads(case):
    return {i for i, _ in reads_of(case.records)}


def text_spans(grain, case):
    """(per record: its first byte, the span of its ID or None, the spans of its numbers, the byte of its separator; the bytes of
    the text) by adding up field lengths"""
    out, at = [], 0
    recs = case.records
    for p, r in enumerate(recs):
        start, id_span = at, None
        if p == 0 or recs[p - 1][0] != r[0]:
            id_span = (at, at + len(case.ids[r[0]]))
            at = id_span[1] + 1
        numbers = []
        for v in r[1:]:
            numbers.append((at, at + len(str(v))))
            at = numbers[-1][1] + 1
        out.append((start, id_span, numbers, at - 1))
    return out, at


def text_window_coverage(grain, case, T):
    """which of WINDOW_KINDS the case holds: the window edges of every tile are computed from the text's spans"""
    spans, total = text_spans(grain, case)
    cap = text_cap(T)
    found = set()
    for t in range(0, len(spans), T):
        B = spans[t][0]
        E = spans[t + T][0] if t + T < len(spans) else total
        W = [w for w in range((B & ~15) + cap, E, cap)]
        if E - B > 2 * cap:
            found.add("two_caps")
        for start, id_span, numbers, sep in spans[t:t + T]:
            for w in W:
                if id_span and id_span[0] < w < id_span[1]:
                    found.add("short_id" if id_span[1] - id_span[0] <= 64 else "long_id")
                if any(a < w < b for a, b in numbers):
                    found.add("digits")
                if sep == w - 1:
                    found.add("separator")
    return found


def big_text(n=1_048_578, seed=5):
    """(records as an ASSIGN_DTYPE array, (ID bytes, offsets), ids): n records at the taxid grain over reads of one or two
    records, every read with an ID of one to three bytes, built with numpy"""
    from mtsv_tools_amd import _lib
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 3, n)                                                    # more reads than needed, cut to n records
    ends = np.cumsum(sizes)
    n_reads = int(np.searchsorted(ends, n)) + 1
    sizes = sizes[:n_reads].copy()
    sizes[-1] -= int(ends[n_reads - 1]) - n
    read = np.repeat(np.arange(n_reads, dtype=np.uint64), sizes)
    first = np.r_[True, read[1:] != read[:-1]]
    rec = np.zeros(n, dtype=_lib.ASSIGN_DTYPE)
    rec["read"] = read
    rec["tax_id"] = np.where(first, rng.integers(0, 50, n), rng.integers(50, 100000, n))   # ascending inside a read
    rec["edit"] = rng.integers(0, 12, n)
    id_len = rng.integers(1, 4, n_reads)
    slots = np.zeros((n_reads, 4), dtype=np.uint8)                                   # the ID, one NUL, and what the mask drops
    slots[:, :3] = rng.integers(ord("a"), ord("z") + 1, (n_reads, 3))
    cols = np.arange(4)[None, :]
    slots[cols == id_len[:, None]] = 0
    blob = slots[cols <= id_len[:, None]].tobytes()
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(id_len + 1, out=off[1:])
    ids = blob.decode().split("\0")[:-1]
    return rec, (blob, off), ids


def big_text_expected(rec, ids):
    return TC.text(F.TAXID, list(zip(rec["read"].tolist(), rec["tax_id"].tolist(), rec["edit"].tolist())), ids)


# ---- parser ---------------------------------------------------------------------------------------------------------------------
PARSE_SIDES = (-1, 0, 1, 2)       # a token start at m + d has its ',' at m + d - 1: the side d = 2 puts a ',' at m + 1
PARSE_FLOOR = 64
BIG = "4294967295-4294967295-4294967295=4294967295"                                  # 43 bytes


def _number(rng, digits):
    return str(rng.randrange(10 ** (digits - 1) if digits > 1 else 0, min(10 ** digits, 1 << 32)))


def _token(rng, tax, length):
    """T-G-O=E of exactly `length` bytes, 7 .. 34 for a TaxID of one digit"""
    rest = length - len(str(tax)) - 3
    assert 3 <= rest <= 30
    g = rng.randrange(max(1, rest - 20), min(10, rest - 2) + 1)
    o = rng.randrange(max(1, rest - g - 10), min(10, rest - g - 1) + 1)
    return f"{tax}-{_number(rng, g)}-{_number(rng, o)}={_number(rng, rest - g - o)}"


def _exact_line(rng, n):
    """a line of exactly n bytes, 7 .. 314: tokens with the TaxIDs 1, 2, ..."""
    k = -(-(n + 1) // 35)
    assert n >= 7 and k <= 9
    total = n - (k - 1)
    return ",".join(_token(rng, i + 1, total // k + (i < total % k)) for i in range(k))


def _base_line(rng):
    """a line as parse_cases.edge_lines makes them: 1 to 8 long tokens, keys ascending; now and then an empty line"""
    if rng.random() < 0.03:
        return ""
    V = PC.VALUES
    keys = set()
    for _ in range(rng.randrange(1, 9)):
        tax = rng.choice(V[:6]) if rng.random() < 0.7 else rng.choice(V)
        keys.add((tax, rng.choice(V[:4] + V[-3:]), rng.choice(V)))
    return ",".join(f"{t}-{g}-{o}={rng.choice(V)}" for t, g, o in sorted(keys))


class _Text:
    def __init__(self, rng):
        self.rng, self.lines, self.at, self.read = rng, [], 0, 0

    def push(self, hits):
        self.read += self.rng.randrange(1, 4)
        self.lines.append((self.read, hits))
        self.at += len(hits)

    def fill_to(self, pos):
        """lines until the text has exactly `pos` bytes (0 or at least 7 more than it has)"""
        while self.at != pos:
            gap = pos - self.at
            assert gap >= 7, (pos, self.at)
            line = _base_line(self.rng)
            if len(line) == gap or len(line) <= gap - 7:
                self.push(line)
            elif gap > 300:
                self.push(_exact_line(self.rng, 100))
            else:
                self.push(_exact_line(self.rng, gap))

    def start_at(self, pos, token=None):
        """a line whose second token starts at byte `pos`, behind a ','"""
        self.fill_to(pos - 8)
        self.push(_token(self.rng, 1, 7) + "," + (token or _token(self.rng, 2, self.rng.randrange(7, 35))))


def parse_spacing(T):
    return max(T, 256)


@functools.lru_cache(maxsize=None)
def parse_texts(T):
    """{name: lines}: per side d of PARSE_SIDES token starts behind a ',' at m + d for every edge m (side); the 43-byte token
    with 1, 21 and 42 of its bytes in front of a tile edge, inside a run of equal (TaxID, GI) that goes on behind the edge
    (straddle); a non-empty line on a tile's first byte, behind no, one and three empty lines (lines); from s(T) = 16 on lines
    of T=E tokens of three bytes, for the taxid grain alone (short)"""
    rng = random.Random(5000 + T)
    out = {}
    for d in PARSE_SIDES:
        t = _Text(rng)
        for p in targets(T, d, floor=PARSE_FLOOR):
            t.start_at(p)
        t.fill_to(max(3 * T, t.at) + 60)
        out[f"side{d:+d}"] = t.lines
    sp = parse_spacing(T)
    t = _Text(rng)
    for k, front in enumerate((1, 21, 42), 1):
        t.fill_to(k * sp - front - 43)
        t.push(",".join([_token(rng, 1, 7), BIG[:-12] + "0=5", BIG, BIG[:-10] + "7"]))
    t.fill_to(max(3 * T, 3 * sp) + 60)
    out["straddle"] = t.lines
    t = _Text(rng)
    for k, empty in enumerate((0, 1, 3), 1):
        t.fill_to(k * sp)
        for _ in range(empty):
            t.push("")
        t.push(_exact_line(rng, 30))
    t.fill_to(max(3 * T, 3 * sp) + 60)
    out["lines"] = t.lines
    if stretch(T) >= 16:
        t = _Text(rng)
        while t.at < 3 * T + 20:
            t.push(",".join(f"{k}={rng.randrange(10)}" for k in range(10)))
        out["short"] = t.lines
    return out


def parse_grains(name):
    return (F.TAXID,) if name == "short" else (F.TAXID, F.TAXID_GI, F.LONG)


def parse_refused(T):
    """(lines, the line to be named): a token outside the grammar that starts 20 bytes in front of the second tile edge"""
    t = _Text(random.Random(4000 + T))
    t.start_at(2 * T - 20, "2-1-x=2")
    bad = len(t.lines) - 1
    t.fill_to(3 * T + 60)
    return t.lines, bad


def parse_coverage(lines):
    """from the lines alone: the bytes at which a token starts behind a ',' (starts), at which a ',' stands (commas), at which a
    non-empty line begins (line_starts), {offset: empty lines that share it} (empty), [(first byte, token)] (tokens) and per
    line the token starts (by_line)"""
    cov = {"starts": set(), "commas": set(), "line_starts": set(), "empty": {}, "tokens": [], "by_line": [], "bytes": 0}
    at = 0
    for _, h in lines:
        row = []
        if h == "":
            cov["empty"][at] = cov["empty"].get(at, 0) + 1
        else:
            cov["line_starts"].add(at)
            p = at
            for k, tok in enumerate(h.split(",")):
                if k:
                    cov["commas"].add(p - 1)
                    cov["starts"].add(p)
                cov["tokens"].append((p, tok))
                row.append((p, tok))
                p += len(tok) + 1
        cov["by_line"].append(row)
        at += len(h)
    cov["bytes"] = at
    return cov
