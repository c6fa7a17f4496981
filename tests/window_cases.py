"""Long merged windows of non-repeating text ("stepping stones"), placed at the edges of the verify kernels' window
stores: the rings of k_sw_pairs (512 columns) and k_evaluate (1024), refilled half a ring at a time, and the sector stream
of k_edit_myers.  Pure Python: the database, the reads and what each read is planned to do; nothing of the product.

The construction.  With seed_size = seed_interval = 18 (SEED) the seeds of a read sit in slots at offsets 0, 18, 36, ...
and do not overlap.  A read of L bases starts as the body text[P : P + L]; ED = ceil(L * rate), w = L + 2 * ED.  A slot
overwritten with the 18 bases at text position X is one exact seed hit, a stone, whose window starts at X - q - ED (q the
slot's offset).  Head stones take the first slots and put their windows s1, s1 + s2, ... columns before the body's, tail
stones take the last slots and put theirs behind it; every step is below w, so the windows chain (add_seed_hit) into one
candidate of exactly w + sum(steps) columns.  The body aligns ED + sum(head steps) columns into it: at its end with head
stones only, at its start with tail stones only.  A stone costs the read about 10 edits, 18 at most; stone_budget() keeps
a rung that is meant to hit a stone or more below ED.  revcomp(read) has the same window on strand 1.

A clean body is decided by the bound of k_edit_myers before any sweep, so the rungs come a second time, in the groups named
"...u", with reads whose distance ends between ED and 2 * ED and whose score still passes (undecided_gap): those reach the
sweep of k_sw_pairs."""
import hashlib
import math
import random

import helpers
from helpers import revcomp, rnd_seq

K = 18
SEED = dict(seed_size=K, seed_interval=K)
RING_PAIRS, RING_EVAL = 512, 1024

# ---- the database ----------------------------------------------------------------------------------------------------------
N_RUNS = (2, 4, 7, 9, 12)         # run k of the N sequence holds N_RUNS[k] N from N_FIRST + k * N_EVERY on; further
N_FIRST, N_EVERY = 1800, 1800    # apart than the windows laid over them are long, so that a window holds one run
CHAINS = {150: ("BCAG", "AC", "CCG", "B"), 253: ("BCG", "AB")}  # helpers.chain_copy kinds, one TaxID per chain


class Database:
    """entries (tax_id, gi, sequence) in text order; start[name] / seq[name] of the named sequences:
    "first"  3 000 bases from text position 0: a chain that starts near its first base is clipped at bin.start
    "main"   16 000 random bases
    "n"      11 000 bases with runs of 2..12 N at N_FIRST + k * N_EVERY
    chains   damaged copies of one segment per TaxID (helpers.chain_copy): candidates with successors
    "last"   4 000 bases that end the text: a chain that ends at its last base is clipped at bin.end, within the last 63
             symbols of the text"""

    def __init__(self):
        rng = random.Random(0x57E9)
        n_seq = bytearray(helpers._fast_seq(rng, 11000))
        for k, run in enumerate(N_RUNS):
            n_seq[N_FIRST + k * N_EVERY:N_FIRST + k * N_EVERY + run] = b"N" * run
        named = [("first", 11, helpers._fast_seq(rng, 3000)), ("main", 12, helpers._fast_seq(rng, 16000)), ("n", 13, bytes(n_seq))]
        self.chain_reads = {}
        tax = 700
        for L, chains in CHAINS.items():
            sh = helpers.CHAIN_SHAPES[L]
            self.chain_reads[L] = []
            for kinds in chains:
                seg = rnd_seq(rng, helpers.CHAIN_LO + sh["region"] + 180)
                for k, kind in enumerate(kinds):
                    copy = helpers.chain_copy(rng, seg, kind, L)
                    named.append(("chain%d-%s-%d" % (L, kinds, k), tax, rnd_seq(rng, rng.randrange(80, 201)) + copy + rnd_seq(rng, rng.randrange(80, 201))))
                tax += 1
                for k in range(6):
                    st = helpers.CHAIN_LO - rng.randrange(sh["back"][0], sh["back"][1] + 1)
                    r = seg[st:st + L]
                    self.chain_reads[L].append(r if k % 2 == 0 else revcomp(r))
        named.append(("last", 15, helpers._fast_seq(rng, 4000)))
        self.entries = [(tax, 100 + i, s) for i, (name, tax, s) in enumerate(named)]
        self.text = b"".join(s for _, _, s in named)
        self.seq, self.start, at = {}, {}, 0
        for name, _, s in named:
            self.seq[name], self.start[name] = s, at
            at += len(s)
        self.n = at + 1  # symbols of the text with its sentinel

    def bin_of(self, name):
        return self.start[name], self.start[name] + len(self.seq[name])


_db = None


def database():
    global _db
    if _db is None:
        _db = Database()
    return _db


# ---- one read ----------------------------------------------------------------------------------------------------------------
def edit_budget(L, rate):
    return math.ceil(L * rate)


def n_slots(L):
    return (L - K) // K + 1


def stone_budget(L, rate):
    """the stones a read may carry and still hit nearly always: about 10.5 edits a stone, a stone or more below ED"""
    return max(0, (edit_budget(L, rate) - 6) // 11)


def split_steps(total, m, w):
    """total columns over m steps that differ by one at most, every one of them below w"""
    if m == 0:
        assert total == 0
        return []
    steps = [total // m + (1 if k < total % m else 0) for k in range(m)]
    assert 0 < min(steps) and max(steps) < w, (total, m, w)
    return steps


class Read:
    """seq: the read as it is given to the binner (reverse-complemented on strand 1); sites: [(text position, read offset)]
    of its planned exact seed hits, stones and body, on the forward strand; P: text position of the body; window: the
    planned (start, end) before any clipping at the bin"""

    def __init__(self, seq, strand, P, sites, window, body_col):
        self.seq, self.strand, self.P, self.sites, self.window, self.body_col = seq, strand, P, sites, window, body_col


def stepping_stones(text, P, L, rate, head, tail, strand=0, subs=0, rng=None, gap=0):
    """the read of L bases whose body is text[P : P + L], with len(head) head stones and len(tail) tail stones; head[0] and
    tail[0] are the steps next to the body.  subs substitutions in the first 60 bases of the body that no stone covers.
    gap: the body leaves out that many bases of the text, one half in front of the slot a third into the body's slots and
    the other in front of the slot two thirds into them (and goes on as far behind P + L): three pieces, and the windows of
    the seeds behind a gap lie as many columns further on, like a step."""
    ED = edit_budget(L, rate)
    w = L + 2 * ED
    assert len(head) + len(tail) < n_slots(L) and all(0 < s < w for s in list(head) + list(tail) + [gap or 1])
    mh, mt = len(head), len(tail)
    nb = n_slots(L) - mh - mt
    cuts = ((K * (mh + nb // 3), gap // 2), (K * (mh + 2 * nb // 3), gap - gap // 2))

    def skipped(q):  # bases of the text left out in front of read offset q
        return sum(g for at, g in cuts if q >= at)

    read = bytearray(text[P + q + skipped(q)] for q in range(L))
    sites = {}
    for j in range(n_slots(L)):
        sites[K * j] = P + K * j + skipped(K * j)
    for j in range(mh):  # slot j: its window sum(head[:mh - j]) columns before the body's
        q = K * j
        sites[q] = P - sum(head[:mh - j]) + q
    for j in range(mt):  # the j-th slot from the end: its window sum(tail[:mt - j]) columns behind the body's
        q = K * (n_slots(L) - 1 - j)
        sites[q] = P + gap + sum(tail[:mt - j]) + q
    for q, X in sites.items():
        assert X >= 0 and X + K <= len(text), (P, q, X)
        read[q:q + K] = text[X:X + K]
    if subs:
        read = bytearray(helpers.substitute(rng, bytes(read), subs, lo=K * mh, hi=K * mh + 60))
        lo = K * mh
        sites = {q: X for q, X in sites.items() if q + K <= lo or q >= lo + 60}  # (a slot that holds a change may be lost)
    window = (P - ED - sum(head), P + gap + L + ED + sum(tail))
    seq = bytes(read)
    return Read(revcomp(seq) if strand else seq, strand, P, sorted((X, q) for q, X in sites.items()), window, ED + sum(head))


# ---- rungs -------------------------------------------------------------------------------------------------------------------
class Rung:
    """n reads of L bases at rate, alternately on strand 0 and 1, whose window is planned to be W columns long.
    where: "main" | "n" (an N run across column n_col of the window, counted from its end if n_from_end) |
    "first" (clipped at bin.start) | "last" (clipped at bin.end).  must_hit: the stones stay within stone_budget.
    subs: read k carries k % 10 substitutions in the first 60 bases of its body.
    gap: the body leaves out that many bases of the text, in two halves (undecided_gap(): windows that reach the sweep)."""

    def __init__(self, group, L, rate, head, tail, n=8, where="main", n_col=None, n_from_end=False, subs=False, gap=0, tag=""):
        self.group, self.L, self.rate, self.head, self.tail, self.n = group, L, rate, list(head), list(tail), n
        self.where, self.n_col, self.n_from_end, self.subs, self.gap = where, n_col, n_from_end, subs, gap
        self.ED = edit_budget(L, rate)
        self.w = L + 2 * self.ED
        self.W = self.w + sum(self.head) + sum(self.tail) + gap
        self.body_col = self.ED + sum(self.head)
        self.clipped = where in ("first", "last")
        self.must_hit = not subs and not gap and len(self.head) + len(self.tail) <= stone_budget(L, rate)
        self.name = "L%d-r%s-W%d-%d+%d%s%s" % (L, rate, self.W, len(self.head), len(self.tail), "-gap%d" % gap if gap else "", tag)

    def __repr__(self):
        return self.name

    def _free_of_seeds(self, lo, hi):
        """no stone and no part of the body lies in columns [lo, hi) of the window"""
        cols = [(self.body_col, self.body_col + self.L + self.gap)]
        mh, mt, ns = len(self.head), len(self.tail), n_slots(self.L)
        end = self.body_col + self.gap
        cols += [(self.body_col - sum(self.head[:mh - j]) + K * j, self.body_col - sum(self.head[:mh - j]) + K * j + K) for j in range(mh)]
        cols += [(end + sum(self.tail[:mt - j]) + K * (ns - 1 - j), end + sum(self.tail[:mt - j]) + K * (ns - j)) for j in range(mt)]
        return all(b <= lo or a >= hi for a, b in cols)

    def reads(self):
        d = database()
        rng = random.Random(int.from_bytes(hashlib.sha256(("%s/%s" % (self.group, self.name)).encode()).digest()[:6], "big"))
        before, behind = self.ED + sum(self.head), self.L + self.ED + sum(self.tail) + self.gap
        lo, hi = d.bin_of("main" if self.where == "main" else self.where)
        out = []
        for k in range(self.n):
            if self.where == "main":
                P = rng.randrange(lo + before, hi - behind + 1)
            elif self.where == "first":  # the first stone 0 .. ED - 1 bases into the sequence: ED .. 1 columns clipped
                assert self.head
                P = lo + sum(self.head) + (k * 7) % self.ED
            elif self.where == "last":  # the last stone's window ends 1 .. ED columns behind the sequence
                assert self.tail
                P = hi - behind + 1 + (k * 7) % self.ED
                assert P + self.gap + sum(self.tail) + K * n_slots(self.L) <= hi
            else:  # run k of the N sequence begins a column before the boundary (two, from 4 N on)
                run = N_RUNS[k % len(N_RUNS)]
                at = lo + N_FIRST + (k % len(N_RUNS)) * N_EVERY
                back = 1 if run < 4 else 2
                col = self.W - self.n_col - (run - back) if self.n_from_end else self.n_col - back
                assert self._free_of_seeds(col, col + run), (self.name, col, run)
                P = at - col + before
                assert lo + before <= P <= hi - behind
            out.append(stepping_stones(d.text, P, self.L, self.rate, self.head, self.tail, strand=k % 2,
                                       subs=k % 10 if self.subs else 0, rng=rng, gap=self.gap))
        return out


def undecided_gap(L, rate, stones):
    """A candidate whose distance D lies in ED < D <= 2 * ED is left undecided by k_edit_myers as the bound: in the reference
    order only such a window reaches the sweep of k_sw_pairs.  A stone costs the read 18 of its score and about 9 edits, a
    gap of g bases g of each (ssw: a gap of g costs g), and the L mod 18 bases behind a tail stone are lost to the score:
    with all that at 2 * ED - 4 the local alignment still scores L - 2 * ED + 4, so the sweep must pass the window (the
    oracle's n_edit counts it), which it can only where its ring holds the columns of all pieces of the body.  The gap comes in two halves, the body in three pieces: a piece of p bases can
    also be laid against the text beside its neighbour for about p / 2 edits, so one gap between two halves of the body
    would leave D at a quarter of the read, below ED at rate 0.3; no way round two of three pieces is as cheap.  Whether D
    ends above ED is the oracle's to say: test_long_windows_cpu.py counts the reads that are refused."""
    g = 2 * edit_budget(L, rate) - K * stones - (L - K * n_slots(L)) - 4
    assert g > 0
    return g


def _positions(L, rate, W, group, n=8, undecided=False):
    """the rungs of window length W with the body at its end, at its start and in its middle, with the fewest stones that
    reach W; undecided: and the gap of undecided_gap() in the body"""
    ED = edit_budget(L, rate)
    w = L + 2 * ED
    out = []
    for pos in ("end", "start", "middle"):
        m = 2 if pos == "middle" or undecided else 1  # (undecided: two stones at least keep D well above ED)
        while W - w - (undecided_gap(L, rate, m) if undecided else 0) > m * (w - 1):
            m += 1
        gap = 0
        if undecided:  # (a short window has no room for all of the gap: the steps keep 20 columns each)
            gap = min(undecided_gap(L, rate, m), W - w - 20 * m)
            assert gap + 9 * m > ED + 4, (L, rate, W, m, gap)  # (about 9 edits a stone)
        steps = split_steps(W - w - gap, m, w)
        head, tail = {"end": (steps, []), "start": ([], steps), "middle": (steps[:m // 2], steps[m // 2:])}[pos]
        out.append(Rung(group, L, rate, head, tail, n=n, gap=gap, tag="-" + pos))
    return out


PAIRS_LENGTHS = (511, 512, 513, 767, 768, 769, 1023, 1024, 1025)
EVAL_LENGTHS = (1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049)


def _symmetric(group, L, rate, col, lead=70, **kw):
    """stones on both sides: the body begins `lead` columns before column col of the window, and ends as far behind
    column col counted from the window's end"""
    ED = edit_budget(L, rate)
    w = L + 2 * ED
    side = col - lead - ED
    m = -(-side // (w - 1))
    return Rung(group, L, rate, split_steps(side, m, w), split_steps(side, m, w), **kw)


def _groups():
    g = {}
    # reads of at most 253 bases: k_sw_pairs (ring 512), k_edit_myers (sector stream), MTSV_SW=packed k_evaluate (ring 1024)
    g["p150"] = [r for W in PAIRS_LENGTHS for r in _positions(150, 0.3, W, "p150")]  # (1023..1025: four stones, past the budget)
    g["p253a"] = [r for W in PAIRS_LENGTHS for r in _positions(253, 0.13, W, "p253a")]  # (1023..1025: three stones, past the budget)
    g["p253b"] = [r for W in PAIRS_LENGTHS + (2021,) for r in _positions(253, 0.3, W, "p253b")]
    # (undecided: past 769 columns these two would need more stones than leave room for a gap that keeps D above ED)
    g["p150u"] = [r for W in PAIRS_LENGTHS[:6] for r in _positions(150, 0.3, W, "p150u", undecided=True)]
    g["p253au"] = [r for W in PAIRS_LENGTHS[:6] for r in _positions(253, 0.13, W, "p253au", undecided=True)]
    g["p253bu"] = [r for W in PAIRS_LENGTHS + (2021,) for r in _positions(253, 0.3, W, "p253bu", undecided=True)]
    g["p96"] = [r for W in (460, 511, 512, 513) for r in _positions(96, 0.3, W, "p96")]  # (three words; from 511 on past the budget)
    # the body across a refill boundary of the pairs ring, N runs across one, windows clipped at the bin: 150 and 253 bases
    sp = [_symmetric("p-edges", 253, 0.3, 512, tag="-across512"), _symmetric("p-edges", 253, 0.3, 768, tag="-across768")]
    for col in (512, 768):
        for from_end in (False, True):
            head, tail = ([380], [380, 380]) if from_end else ([380, 380], [380])
            sp.append(Rung("p-edges", 253, 0.3, head, tail, n=10, where="n", n_col=col, n_from_end=from_end,
                           tag="-N%d%s" % (col, "e" if from_end else "s")))
    sp += [Rung("p-edges", 253, 0.3, [300, 350, 404], [], where="first", tag="-first"),
           Rung("p-edges", 253, 0.3, [], [300, 350, 404], where="last", tag="-last")]
    g["p-edges"] = sp
    # the same edges on windows that reach the sweep of k_sw_pairs
    su = [_symmetric("p-edges-u", 253, 0.3, 512, gap=undecided_gap(253, 0.3, 2), tag="-across512"),
          _symmetric("p-edges-u", 253, 0.3, 768, gap=undecided_gap(253, 0.3, 4), tag="-across768")]
    for col in (512, 768):
        for from_end in (False, True):
            head, tail = ([380], [380, 380]) if from_end else ([380, 380], [380])
            su.append(Rung("p-edges-u", 253, 0.3, head, tail, n=10, where="n", n_col=col, n_from_end=from_end,
                           gap=undecided_gap(253, 0.3, 3), tag="-N%d%s" % (col, "e" if from_end else "s")))
    su += [Rung("p-edges-u", 253, 0.3, [300, 350, 404], [], where="first", gap=undecided_gap(253, 0.3, 3), tag="-first"),
           Rung("p-edges-u", 253, 0.3, [], [300, 350, 404], where="last", gap=undecided_gap(253, 0.3, 3), tag="-last")]
    g["p-edges-u"] = su
    g["p150-edges"] = [Rung("p150-edges", 150, 0.3, [200, 230, 239], [], where="first", tag="-first"),
                       Rung("p150-edges", 150, 0.3, [], [200, 230, 239], where="last", tag="-last"),
                       Rung("p150-edges", 150, 0.3, [239, 239], [120], where="first", tag="-first-mid"),
                       Rung("p150-edges", 150, 0.3, [239, 239], [200], n=10, where="n", n_col=512, tag="-N512s"),
                       Rung("p150-edges", 150, 0.3, [200], [239, 239], n=10, where="n", n_col=512, n_from_end=True, tag="-N512e")]
    # reads of 254 bases and more: k_evaluate (ring 1024), the register word kernel up to 256, the tiled kernel beyond
    for L in (254, 256, 257, 300):
        g["e%d" % L] = [r for W in EVAL_LENGTHS for r in _positions(L, 0.3, W, "e%d" % L, n=4)]
    g["e600"] = [r for W in EVAL_LENGTHS + (4200,) for r in _positions(600, 0.13, W, "e600", n=4)]
    se = [_symmetric("e300-edges", 300, 0.3, 1024, tag="-across1024"), _symmetric("e300-edges", 300, 0.3, 1536, tag="-across1536")]
    for col in (1024, 1536):
        for from_end in (False, True):
            head, tail = ([400, 400, 400], []) if from_end else ([], [400, 400, 400])
            se.append(Rung("e300-edges", 300, 0.3, head, tail, n=10, where="n", n_col=col, n_from_end=from_end,
                           tag="-N%d%s" % (col, "e" if from_end else "s")))
    se += [Rung("e300-edges", 300, 0.3, [400, 450, 470, 479], [], where="first", tag="-first"),
           Rung("e300-edges", 300, 0.3, [], [400, 450, 470, 479], where="last", tag="-last")]
    g["e300-edges"] = se
    g["e256-edges"] = [_symmetric("e256-edges", 256, 0.3, 1024, tag="-across1024")]
    g["e1000"] = [Rung("e1000", 1000, 0.13, [1259] * 7, [], n=4, tag="-end")]  # 10 073 columns, once
    return g


GROUPS = _groups()
PAIRS_GROUPS = tuple(k for k in GROUPS if k.startswith("p"))
EVAL_GROUPS = tuple(k for k in GROUPS if k.startswith("e"))

# substitutions in the body at the default rate: the three outcomes of the reference's two checks on long windows
SUBS_RUNGS = (Rung("subs", 150, 0.13, [189, 189], [], n=60, subs=True, tag="-subs"),
              Rung("subs", 253, 0.13, [318, 318, 318], [], n=60, subs=True, tag="-subs"),
              Rung("subs", 253, 0.13, [236, 236], [236], n=60, subs=True, tag="-subs"))


def group_rate(group):
    rates = {r.rate for r in GROUPS[group]}
    assert len(rates) == 1
    return rates.pop()


def group_reads(group):
    """the reads of a group, rung after rung"""
    return [rd for r in GROUPS[group] for rd in r.reads()]


def ordinary_reads(rng, L, n, rate=0.13):
    """cuts of the main sequence with 0 .. ED + 20 substitutions, both strands: windows of w columns, a part of them refuted"""
    d = database()
    lo, hi = d.bin_of("main")
    ED = edit_budget(L, rate)
    out = []
    for k in range(n):
        at = rng.randrange(lo, hi - L)
        r = helpers.substitute(rng, d.text[at:at + L], (0, 2, ED - 1, ED + 2, ED + 20)[k % 5])
        out.append(r if k % 2 else revcomp(r))
    return out


def neighbours_batch():
    """at the default rate: one long window (253 bases, 511 .. 1273 columns) in every four reads, beside ordinary reads of
    150 and 253 bases and the reads of the chains, whose refuted candidates have successors"""
    rng = random.Random(0x9E16)
    d = database()
    longs = [rd.seq for r in GROUPS["p253a"] + GROUPS["p253au"] for rd in r.reads()[:2]] + [rd.seq for rd in SUBS_RUNGS[1].reads()[:12]]
    short = d.chain_reads[150] + d.chain_reads[253] + ordinary_reads(rng, 150, 60) + ordinary_reads(rng, 253, 30)
    short += ordinary_reads(rng, 150, max(0, 3 * len(longs) - len(short)))
    rng.shuffle(short)
    rng.shuffle(longs)
    out = []
    for k, r in enumerate(longs):  # the long window takes each place of a quad in turn
        three = short[3 * k:3 * k + 3]
        out += three[:k % 4] + [r] + three[k % 4:]
    return out + short[3 * len(longs):]
