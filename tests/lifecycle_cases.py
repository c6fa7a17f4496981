"""Seeded operation sequences on a few long-lived handles: sequence(kind, seed) returns a list of steps as plain data (dicts of
ints, strings, tuples and lists).  lifecycle_model.py says what every step must give; test_lifecycle.py replays the list on
the device; test_lifecycle_cpu.py asserts what the list must contain (the coverage table).  No device, no library code.

kind "fold": three source folds, one per grain ("taxid", "taxid_gi", "long"), an output fold "out" at the TAXID grain that
every lca and pair call writes, a fold of representatives "rep" and the map of identical reads.  The sequence walks every
source fold through five contents -- middling, large, small, empty, something again -- and runs the calls that own scratch
memory on each of them, so that every such call meets a smaller input after a larger one and an empty one between two that are
not.  Sizes come from LADDER.  Every step draws its keys from a pool of its own (TaxIDs, offsets, edits), so what an
earlier, larger call left in memory cannot coincide with what a later call must produce.

To add an operation: emit its step here (a dict with "op", the handle "h" and its arguments), give FoldModel.apply and
FoldModel.refusal its sentence of the header, replay it in test_lifecycle.py, and name it in test_lifecycle_cpu.OWNERS if it
owns scratch memory.

step            fields
reset           h, n_reads
add_records     h, records
add_text        h, lines [(read, hits)]
lca             h, slack, out
pair            h, mode, max_insert, unpaired, out
take            reads [bytes]                 (upload + take_unique: fills the map)
expand          h (the destination), src
format_text     h, n_ids                      (only inside a refusal: the observers format every touched fold anyway)
refuse          call (one of the above), code, why
"""
import os
import random

import fold_ref as F
import lca_ref as LR
import pair_ref as PR

E_ARG, E_FORMAT = -1, -3
SLACK_ALL = 0xffffffff
FOLDS = {"taxid": F.TAXID, "taxid_gi": F.TAXID_GI, "long": F.LONG, "out": F.TAXID}
SOURCES = ("taxid", "taxid_gi", "long")
# records and reads: 0, 1, 63/64/65; the 1024-element floor of a scratch array; a few tiles; both sides of a fold's first
# allocation (65 536 records); one list that needs the second
LADDER = (0, 1, 63, 64, 65, 1023, 1025, 4097, 65535, 65537, 140004)
FOLD_SEEDS = (1, 2, 3)
TAXONOMY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nodes_primates.dmp")
_listed = []


def listed_taxa():
    if not _listed:
        _listed.extend(LR.Taxonomy(open(TAXONOMY).read()).listed)
    return _listed


def pool_of(rng, salt, size):
    """a step's own TaxIDs: mostly nodes of the taxonomy, a few it does not know, one with bit 31 set"""
    known = rng.sample(listed_taxa(), min(size, 40))
    return known + [1000003 + 1000 * salt + k for k in range(max(2, size - len(known)))] + [(1 << 31) + salt]


def key_of(grain, read, rng, pool):
    t = rng.choice(pool)
    if grain == F.TAXID:
        return (read, t)
    g = rng.randrange(1, 3)
    return (read, t, g) if grain == F.TAXID_GI else (read, t, g, rng.randrange(0, 3000))


def finish(grain, keys, rng):
    if grain == F.TAXID_GI:
        return [(*k, rng.randrange(0, 3000), rng.randrange(0, 7)) for k in sorted(keys)]
    return [(*k, rng.randrange(0, 7)) for k in sorted(keys)]


def gen_records(grain, n_reads, n, rng, salt):
    """n records of distinct keys over the reads below n_reads; an eighth of them planted as mates 2p and 2p + 1 that share
    a TaxID, a GI and (LONG) lie within 150 bases of each other"""
    pool = pool_of(rng, salt, max(10, (3 * n) // max(n_reads, 1)))
    keys = set()
    for _ in range(n // 16 if n_reads >= 2 else 0):
        p, t, g, o = rng.randrange(n_reads // 2), rng.choice(pool), rng.randrange(1, 3), rng.randrange(0, 3000)
        for mate in (0, 1):
            k = (2 * p + mate, t, g, o + mate * rng.randrange(0, 150))
            keys.add(k[:2] if grain == F.TAXID else k[:3] if grain == F.TAXID_GI else k)
    while len(keys) > n:
        keys.pop()
    last = None
    while len(keys) < n:
        if last is not None and grain != F.TAXID and rng.random() < 0.45:
            # the same read and TaxID again: runs of several records, which straddle the tiles of the passes that reduce them
            last = (last[0], last[1], rng.randrange(1, 4)) + ((rng.randrange(0, 3000),) if grain == F.LONG else ())
        else:
            last = key_of(grain, rng.randrange(n_reads), rng, pool)
        keys.add(last)
    return finish(grain, keys, rng)


def gen_two_per_read(grain, n_reads, rng, salt):
    """two records for every read, nearly always of different TaxIDs, from a pool so wide that mates seldom share one:
    PAIR_EITHER keeps nearly every record"""
    pool = pool_of(rng, salt, 70)
    keys = set()
    for r in range(n_reads):
        two = rng.sample(pool, 2)
        if grain != F.TAXID and rng.random() < 0.05:  # (a run of two records: some runs straddle a tile of any size)
            two[1] = two[0]
        for g, t in enumerate(two, 1):
            keys.add((r, t) if grain == F.TAXID else (r, t, g) if grain == F.TAXID_GI else (r, t, g, rng.randrange(0, 800)))
    return finish(grain, keys, rng)


def token(grain, rec, rng):
    if grain == F.TAXID:
        _, t, e = rec
        return rng.choice((f"{t}={e}", f"{t}-{rng.randrange(1, 9)}={e}", f"{t}-{rng.randrange(1, 9)}-{rng.randrange(0, 99)}={e}"))
    _, t, g, o, e = rec
    return f"{t}-{g}-{o}={e}"


def worse(grain, rec, rng):
    """a record of the same key that loses against rec"""
    if grain == F.TAXID_GI:
        return (*rec[:3], rec[3] + rng.randrange(0, 5), rec[4] + rng.randrange(1, 4))
    return (*rec[:-1], rec[-1] + rng.randrange(1, 4))


def gen_lines(grain, recs, n_reads, rng):
    """result lines that hold the records, some keys more than once (the better value first or last), some lines empty"""
    lines, by_read = [], {}
    for r in recs:
        by_read.setdefault(r[0], []).append(r)
    empty = set(rng.sample(range(n_reads), min(n_reads, 3))) - set(by_read) if n_reads else set()
    for read in sorted(set(by_read) | empty):
        toks = []
        for r in by_read.get(read, []):
            run = [r] + ([worse(grain, r, rng)] if rng.random() < 0.2 else [])
            rng.shuffle(run)
            toks += [token(grain, x, rng) for x in run]
        lines.append((read, ",".join(toks)))
    return lines


def seq_of(g, length=14):
    return bytes(b"ACGT"[(g >> (2 * k)) & 3] for k in range(length))


def gen_take(n, rng, salt):
    """n reads of which about half are copies of earlier ones, some in lower case, some cut short"""
    distinct = [seq_of(salt * 100003 + k) for k in range(max(1, n // 2))]
    reads = []
    for j in range(n):
        r = distinct[j] if j < len(distinct) and rng.random() < 0.7 else rng.choice(distinct)
        reads.append(r.lower() if rng.random() < 0.1 else r[:9] if rng.random() < 0.05 else r)
    return reads


class Writer:
    def __init__(self, kind, seed):
        self.kind, self.seed, self.n = kind, seed, 0

    def rng(self):
        """a generator of its own for every step"""
        self.n += 1
        return random.Random(f"{self.kind}-{self.seed}-{self.n}"), self.seed * 1000 + self.n


def interleave(rng, lists):
    """one list that keeps the order inside each of `lists`"""
    lists = [list(l) for l in lists if l]
    out = []
    while lists:
        l = rng.choice(lists)
        out.append(l.pop(0))
        if not l:
            lists.remove(l)
    return out


def fold_sequence(seed):
    w = Writer("fold", seed)
    top, _ = w.rng()
    edge_h = ("taxid", "taxid_gi")[seed % 2]          # the source fold that crosses a fold's first allocation
    edge_first = (65535, 65537)[(seed // 2) % 2]
    rep_h = SOURCES[seed % 3]                         # the grain of the fold of representatives: expand writes this source fold
    reads_of = {
        # n_reads per content: "taxid_gi" numbers an odd count of reads (no pair call), the other two an even one
        "taxid": [top.choice((1022, 1026)), 65538 if edge_h == "taxid" else 4098, top.choice((62, 64, 66)), top.choice((2, 64)), 1024],
        "taxid_gi": [1025, 65537 if edge_h == "taxid_gi" else 4097, top.choice((63, 65)), 1, top.choice((1, 1023))],
        "long": [top.choice((1022, 1026, 4098)), 70002, top.choice((62, 64, 66)), top.choice((2, 64)), top.choice((1022, 1026))],
    }
    records_of = {
        "taxid": [top.choice((1023, 1025)), edge_first if edge_h == "taxid" else 4097, top.choice((63, 64, 65)), 0, top.choice((1023, 1025))],
        "taxid_gi": [1025, edge_first if edge_h == "taxid_gi" else 4097, top.choice((63, 64, 65)), 0, 1],
        "long": [top.choice((1023, 1025, 4097)), 140004, top.choice((63, 64, 65)), 0, top.choice((1023, 1025))],
    }
    if reads_of["taxid_gi"][4] == 1023:
        records_of["taxid_gi"][4] = 1025
    takes = [4097, 65, None, 1025]                    # the reads of the takes after contents 1..4 (None: the map stays, rep is emptied)

    def content(h, c):
        """the steps that give source fold h its content c and run the calls on it"""
        grain, n_reads, n = FOLDS[h], reads_of[h][c], records_of[h][c]
        steps = [{"op": "reset", "h": h, "n_reads": n_reads}]
        rng, salt = w.rng()
        if n == 140004:
            recs = gen_two_per_read(grain, n_reads, rng, salt)
        else:
            recs = gen_records(grain, n_reads, n, rng, salt)
        # the second list: new keys and a third of the first list's keys again, with other values
        rng2, salt2 = w.rng()
        n2 = 0 if n == 0 else 1 if n == 1 else 66 if n in (65535, 65537) else 4097 if c == 1 else min(n, 1025) // 2 + 1
        again = [worse(grain, r, rng2) if rng2.random() < 0.5 else r for r in rng2.sample(recs, min(len(recs), n2 // 3))]
        second = F.fold(grain, gen_records(grain, n_reads, n2, rng2, salt2) if n2 else [], again)
        adds = [{"op": "add_records", "h": h, "records": recs}, {"op": "add_text", "h": h, "lines": gen_lines(grain, second, n_reads, rng2)}]
        if n == 0:                                    # an empty list and lines that hold nothing
            adds[1]["lines"] = [(0, "")] if rng2.random() < 0.5 else []
        elif rng2.random() < 0.5 and n < 65535:
            adds.reverse()
        steps += adds
        calls = []
        if h == "long":                               # every call that owns scratch memory, on every content of this fold
            calls = [{"op": "lca", "h": h, "slack": rng2.choice((0, 1, SLACK_ALL)), "out": "out"}]
            calls += [{"op": "pair", "h": h, "mode": m, "max_insert": rng2.choice((150, 300, 600)), "unpaired": rng2.choice((0, 5)), "out": "out"}
                      for m in (PR.EITHER, PR.BOTH, PR.PROPER)]
            if n != 140004:                           # (the large content: lca, then EITHER, while out is too small for each)
                rng2.shuffle(calls)
        elif h == "taxid":
            calls = [rng2.choice(({"op": "lca", "h": h, "slack": rng2.choice((0, 2)), "out": "out"},
                                  {"op": "pair", "h": h, "mode": rng2.choice((PR.BOTH, PR.EITHER)), "max_insert": 0, "unpaired": 3, "out": "out"}))]
        else:
            calls = [{"op": "lca", "h": h, "slack": rng2.choice((0, 1, SLACK_ALL)), "out": "out"}]
        return steps + calls

    def episode(e):
        """a take, the representatives' records, the expansion into the source fold of rep's grain"""
        grain = FOLDS[rep_h]
        rng, salt = w.rng()
        steps = []
        if takes[e] is not None:
            reads = gen_take(takes[e], rng, salt)
            steps.append({"op": "take", "reads": reads})
            first = {}
            reps = [j for j, r in enumerate(reads) if first.setdefault(r.upper(), j) == j]
            n = takes[e]
            pool = pool_of(rng, salt, 8)
            keys = set()
            for j in reps:
                for _ in range(rng.choice((0, 1, 1, 2, 5))):
                    keys.add(key_of(grain, j, rng, pool))
            steps += [{"op": "reset", "h": "rep", "n_reads": n}, {"op": "add_records", "h": "rep", "records": finish(grain, keys, rng)}]
        else:
            steps.append({"op": "reset", "h": "rep", "n_reads": takes[e - 1]})
        steps.append({"op": "expand", "h": rep_h, "src": "rep"})
        return steps

    def refusals():
        rng, salt = w.rng()
        two = [(0, 9, 1), (0, 7, 1)] if FOLDS[edge_h] == F.TAXID else [(0, 9, 1, 5, 1), (0, 7, 1, 5, 1)]
        return [
            {"op": "refuse", "why": "out of a wide grain", "code": E_ARG, "call": {"op": "lca", "h": "taxid", "slack": 0, "out": "long"}},
            {"op": "refuse", "why": "out of a wide grain", "code": E_ARG, "call": {"op": "pair", "h": "long", "mode": PR.BOTH, "max_insert": 0, "unpaired": 0, "out": "taxid_gi"}},
            {"op": "refuse", "why": "out is the fold itself", "code": E_ARG, "call": {"op": "pair", "h": "taxid", "mode": PR.BOTH, "max_insert": 0, "unpaired": 0, "out": "taxid"}},
            {"op": "refuse", "why": "out is the fold itself", "code": E_ARG, "call": {"op": "lca", "h": "out", "slack": 0, "out": "out"}},
            {"op": "refuse", "why": "an odd n_reads", "code": E_ARG, "call": {"op": "pair", "h": "taxid_gi", "mode": PR.EITHER, "max_insert": 0, "unpaired": 1, "out": "out"}},
            {"op": "refuse", "why": "keys that do not ascend", "code": E_ARG, "call": {"op": "add_records", "h": edge_h, "records": two}},
            {"op": "refuse", "why": "an ID table of another length", "code": E_ARG, "call": {"op": "format_text", "h": rng.choice(SOURCES), "n_ids": 7}},
            {"op": "refuse", "why": "a malformed token", "code": E_FORMAT, "call": {"op": "add_text", "h": rng.choice(SOURCES), "lines": [(0, rng.choice(("5-1-2=1,,7-1-2=2", "5-1-2=", "5-1-2=1,x-1-1=2", "5-1-2=12345678901")))]}},
        ]

    steps = []
    FOLDS_ALL = dict(FOLDS, rep=FOLDS[rep_h])
    for c in range(5):
        lists = {h: content(h, c) for h in SOURCES}
        if c == 1:                                    # the large content of "long" first: out must be too small for it
            steps += lists.pop("long")
        steps += interleave(top, list(lists.values()))
        if c == 2:
            # an edit of 2^31 joins the small content of "taxid": pair refuses the fold until its next reset
            rng, salt = w.rng()
            steps.append({"op": "add_records", "h": "taxid", "records": [(reads_of["taxid"][2] - 1, 4000000000 + salt, 1 << 31)]})
            steps.append({"op": "refuse", "why": "a record with an edit of 2^31", "code": E_ARG,
                          "call": {"op": "pair", "h": "taxid", "mode": PR.EITHER, "max_insert": 0, "unpaired": 1, "out": "out"}})
            steps.append({"op": "lca", "h": "taxid", "slack": 1, "out": "out"})
        if c < 4:
            steps += episode(c)
    # the refusals at seeded places behind the first content (every fold then numbers reads)
    first = next(k for k, s in enumerate(steps) if s["op"] == "take")
    for r in refusals():
        steps.insert(top.randrange(first, len(steps)), r)
    return FOLDS_ALL, steps


# ---- workspaces ------------------------------------------------------------------------------------------------------
# kind "batch": two small databases (helpers.tricky_db), for each a workspace that runs ("runA", "runB") and one that takes the
# input in or filters it ("inA", "inB"), a collector "col" for merge_runs, a fold that takes runs and the map of take_unique.
# The list is written against BatchModel as it goes, so that no step asks for what the header does not define.
#
# step                  fields
# upload                w, reads
# run                   w, params (a name of lifecycle_model.PARAM_SETS)
# run_host              w, reads, params
# run_host_parts        w, parts [reads], params
# set_verify_mode       w, mode         set_assignments   w, mode        set_assignment_grain  w, grain
# set_match_flags       w, mode         set_taxa_report   w, on          taxa_report           w, reset
# take_reads            w, src, keep    copy_reads        w, src         take_unique           w, src
# merge_runs            w, srcs         fold_reset        n_reads        add_run               src
# download_assignments  w, wide         format_text       w, n_ids       (only inside a refusal)
# refuse                call, code, why, says (a piece of the message that names the reason)
# A run, host batch or merge that is written to find nothing carries why_empty, its reason.

BATCH_SEEDS = (1, 2, 3)
DB_SEEDS = {"A": 7, "B": 8}
WORKSPACES = {"inA": "A", "runA": "A", "inB": "B", "runB": "B", "col": "A"}
MAX_READS, MAX_BASES = 4400, 4400 * 330
E_LIMIT = -5
OFF, WITH_HITS, ONLY = 0, 1, 2
_dbs, _oracles = {}, []


def databases():
    import helpers
    if not _dbs:
        for name, seed in DB_SEEDS.items():
            _dbs[name] = helpers.tricky_db(seed=seed)
        # database B also holds twelve of A's sequences under TaxIDs and GIs of its own: reads cut from them hit both, so a
        # read that A's filter matched is not lost on B (two unrelated databases would make half of all chained runs empty)
        entries, gene, unit = _dbs["B"]
        _dbs["B"] = (entries + [(50000 + k, 9000 + k, e[2]) for k, e in enumerate(shared_entries())], gene, unit)
    return _dbs


def shared_entries():
    plain = [e for e in _dbs["A"][0] if len(e[2]) > 1500 and set(e[2]) <= set(b"ACGT")]
    return plain[:12]


def oracles():
    import lifecycle_model as LM
    if not _oracles:
        _oracles.append(LM.Oracles({name: db[0] for name, db in databases().items()}))
    return _oracles[0]


def gen_batch(n, rng, salt, stray=False):
    """n reads, half aimed at each database (helpers.tricky_reads: every corner of the binner), among them an empty read, one
    shorter than a seed and, with stray, one of 400 bases"""
    import helpers
    if n == 0:
        return []
    if n == 1:                                        # (the one read is of a sequence both databases hold)
        return [shared_entries()[salt % 12][2][100:250]]
    reads = []
    for k, name in enumerate(DB_SEEDS):
        entries, gene, unit = databases()[name]
        reads += helpers.tricky_reads(entries, gene, unit, seed=salt * 2 + k, n_each=n // 5 + 2, lengths=(rng.choice((64, 100, 150)),))
    rng.shuffle(reads)
    reads = reads[:n]
    if n >= 8:
        reads[1], reads[2] = b"", b"ACGTACG"
    if stray:
        text = max((e[2] for e in databases()["A"][0]), key=len).upper()
        reads[5] = text[300:700]
    return reads


def gen_nohit(n, rng):
    import helpers
    return [helpers.rnd_seq(rng, 80) for _ in range(n)]


def batch_sequence(seed):
    import lifecycle_model as LM
    w = Writer("batch", seed)
    top, _ = w.rng()
    grains = [(F.TAXID, F.LONG, F.TAXID_GI)[(seed + k) % 3] for k in range(3)]
    model = LM.BatchModel(WORKSPACES, None, grains[0], oracles=oracles())
    steps = []

    expected = []

    def do(**s):
        expected.append(model.apply(s))
        steps.append(s)

    def refuse(why, code, says="", **call):
        do(op="refuse", why=why, code=code, says=says, call=call)

    def run(why_empty=None, **s):
        """a run, a host batch or a merge; why_empty names a step that is written to find nothing"""
        if why_empty:
            s["why_empty"] = why_empty
        do(**s)

    # every grain has a workspace of its own that lives through all five rounds: the collector the fold's, runB the second,
    # runA the third (runA leaves its grain for one host batch in rounds 1 and 3 and comes back)
    grain_of = {"col": grains[0], "runB": grains[1], "runA": grains[2]}
    for name, assign, match, report in (("runA", WITH_HITS, WITH_HITS, True), ("runB", ONLY, WITH_HITS, False), ("col", WITH_HITS, WITH_HITS, True)):
        do(op="set_assignment_grain", w=name, grain=grain_of[name])
        do(op="set_assignments", w=name, mode=assign)
        do(op="set_match_flags", w=name, mode=match)
        if report:
            do(op="set_taxa_report", w=name, on=1)
    do(op="set_match_flags", w="inA", mode=ONLY if seed % 2 else WITH_HITS)
    do(op="fold_reset", n_reads=MAX_READS)
    sizes = [top.choice((1023, 1025)), 4097, top.choice((63, 64, 65)), None, top.choice((1, 1023, 1025))]
    host_sizes = [4097, top.choice((63, 65)), top.choice((1023, 1025)), 0, 64]
    names = ("default", "dense", "stress")
    long_at, grain_at = top.randrange(0, 5), 1
    for r in range(5):
        rng, salt = w.rng()
        batch = gen_nohit(64, rng) if sizes[r] is None else gen_batch(sizes[r], rng, salt, stray=r == 1)
        nothing = "reads that hit nothing" if sizes[r] is None else None
        do(op="upload", w="inA", reads=batch)
        # (the filter runs under the strictest parameters: a read it does not match may still hit its database in the run behind it)
        run(nothing, op="run", w="inA", params="stress")
        presence = model.w["inA"].last["presence"]
        keep = r % 2
        if sizes[r] is not None and not (presence.any() if keep else (~presence).any()):
            keep ^= 1
        if sizes[r] is None:
            keep = 1                                  # nothing survives: every call behind it works on an empty batch
        do(op="take_reads", w="runA", src="inA", keep=keep)
        do(op="copy_reads", w="runB", src="runA")
        do(op="set_verify_mode", w="runA", mode=r % 2)
        small = len(model.w["runA"].reads) <= 1100
        nothing = "no read survived the take" if sizes[r] is None else None
        # (kept unmatched: A's database is asked again under looser parameters; kept matched: B finds the sequences it shares)
        run(nothing, op="run", w="runA", params="default" if not small else names[(r + seed) % 3] if keep else names[(r + seed) % 2])
        run(nothing, op="run", w="runB", params="default" if keep else names[(r + seed + 1) % 3] if small else "stress")
        run(nothing, op="merge_runs", w="col", srcs=["runA", "runB"])
        do(op="add_run", src="col")
        if r == 0:                                    # a host batch through the collector: the fold refuses it, the next merge replaces it
            rng0, salt0 = w.rng()
            run(op="run_host", w="col", reads=gen_batch(65, rng0, salt0), params="default")
            refuse("add_run after a host run", E_ARG, says="host batch", op="add_run", src="col")
        if r % 2:                                     # a run of the collector's own on a copy of the reads: a resident run into the fold
            do(op="copy_reads", w="col", src="runA")
            run(nothing, op="run", w="col", params="default")
            do(op="add_run", src="col")
        if r == 2:                                    # the flags of the collector switched off and on: they speak of no run yet
            do(op="set_match_flags", w="col", mode=OFF)
            do(op="set_match_flags", w="col", mode=WITH_HITS)
        # a host batch through the same workspace, and a take from it
        rng2, salt2 = w.rng()
        host = gen_batch(host_sizes[r], rng2, salt2)
        if r % 2:
            cut = sorted(rng2.sample(range(len(host) + 1), 2)) if host else [0, 0]
            run(None if host else "a batch of zero reads", op="run_host_parts", w="runA", parts=[host[:cut[0]], [], host[cut[0]:cut[1]], host[cut[1]:]],
                params=names[(r + seed + 2) % 3] if len(host) <= 1100 else "default")
        else:
            run(op="run_host", w="runA", reads=host, params=names[(r + seed + 2) % 3] if len(host) <= 1100 else "default")
        if r == 2:                                    # (an ID table of the host batch's own length: only the host batch can be the reason)
            refuse("format_text after a host run", E_ARG, says="host batch", op="format_text", w="runA", n_ids=len(host))
        if host and r in (0, 2, 4):
            do(op="take_reads", w="runB", src="runA", keep=(r // 2) % 2)
            run(op="run", w="runB", params="default")
        # identical reads binned once
        rng3, salt3 = w.rng()
        base = gen_batch([65, 1025, 63, 4097, 1][r], rng3, salt3)
        dups = [rng3.choice(base[:max(1, len(base) // 2)]) if rng3.random() < 0.5 else x for x in base]
        do(op="upload", w="inB", reads=dups)
        do(op="take_unique", w="runB", src="inB")
        run(op="run", w="runB", params="default")
        do(op="taxa_report", w="runA", reset=r % 2)
        do(op="taxa_report", w="col", reset=int(r == 2))
        if r == 3:                                    # a batch of zero reads, resident and from the host
            zero = "a batch of zero reads"
            do(op="upload", w="inA", reads=[])
            run(zero, op="run", w="inA", params="default")
            run(zero, op="run_host", w="runA", reads=[], params="default")
            do(op="upload", w="inB", reads=[])
            do(op="take_unique", w="runB", src="inB")
            run(zero, op="run", w="runB", params="default")
        if r == long_at:
            do(op="upload", w="inB", reads=[b"ACGT" * 8192])
            refuse("a read of 32 768 bases", E_LIMIT, op="run", w="inB", params="default")
        if r in (1, 3):                               # the grain of runA changes: off, another grain, on in the other mode, a host batch, and back
            if r == grain_at:
                refuse("the grain while the assignments are on", E_ARG, op="set_assignment_grain", w="runA", grain=grains[1])
            do(op="set_assignments", w="runA", mode=OFF)
            if r == grain_at:
                refuse("download_assignments while off", E_ARG, op="download_assignments", w="runA", wide=grains[2] != F.TAXID)
            do(op="set_assignment_grain", w="runA", grain=grains[1] if r == 1 else grains[0])
            do(op="set_assignments", w="runA", mode=ONLY if r == 1 else WITH_HITS)
            rng4, salt4 = w.rng()
            run(op="run_host", w="runA", reads=gen_batch(64 if r == 1 else 1025, rng4, salt4), params="default")
            do(op="set_assignments", w="runA", mode=OFF)
            do(op="set_assignment_grain", w="runA", grain=grains[2])
            do(op="set_assignments", w="runA", mode=ONLY if r == 1 else WITH_HITS)
    _expected_batch[seed] = expected
    return {"workspaces": WORKSPACES, "fold_grain": grains[0]}, steps


_expected_batch = {}


def expected_batch(seed):
    """what BatchModel said of every step while the list was written (the list is written against the model)"""
    sequence("batch", seed)
    return _expected_batch[seed]


_cache = {}


def sequence(kind, seed):
    """(handles, steps) of the seeded sequence: the same seed gives the same steps"""
    if (kind, seed) not in _cache:
        _cache[(kind, seed)] = {"fold": fold_sequence, "batch": batch_sequence}[kind](seed)
    return _cache[(kind, seed)]


def brief(step):
    """a step without its data, for messages"""
    s = step["call"] if step["op"] == "refuse" else step
    out = {k: (v if not isinstance(v, (list, tuple)) or (v and isinstance(v[0], str)) else f"<{len(v)}>") for k, v in s.items()}
    return ("refuse " + step["why"] + " ", out) if step["op"] == "refuse" else out
