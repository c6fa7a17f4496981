"""Plain-Python models of long-lived handles: what every observer of a fold (FoldModel) or of a workspace (BatchModel) must
return after every step of an operation sequence (lifecycle_cases.py).  No device, no library code.

The models hold state and nothing else of their own: every derived value comes from the restatements the per-feature tests
use (fold_ref, parse_ref, lca_ref, pair_ref, dedup_ref, assign_ref, grain_ref, taxa_report_ref, chain_ref, chunk_merge_ref)
and, for a workspace, from the CPU oracle's hits.  What an (operation, state) pair returns or refuses is read from
include/mtsv_amd.h; refusal() restates those sentences, and a step the header refuses is never applied.

A record is a tuple of Python ints: (read, tax_id, edit) at the TAXID grain, (read, tax_id, gi, offset, edit) at the wide ones.
"""
import numpy as np

import assign_ref as A
import dedup_ref as D
import fold_ref as F
import grain_ref as GR
import lca_ref as LR
import pair_ref as PR
import parse_ref as TR

E_ARG, E_FORMAT, E_LIMIT = -1, -3, -5  # MTSV_E_*
B31 = 1 << 31
ASSIGN = np.dtype({"names": ["read", "tax_id", "edit"], "formats": ["<u8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 16})
ASSIGN_GI = np.dtype({"names": ["read", "tax_id", "gi", "offset", "edit"], "formats": ["<u8", "<u4", "<u4", "<u4", "<u4"],
                      "offsets": [0, 8, 12, 16, 20], "itemsize": 24})
FIRST_ALLOCATION = 1 << 16  # records a fold's two arrays hold when they are first made (the accumulator's growth)


def as_array(grain, recs):
    """records as the structured array the library takes and returns (padding zero)"""
    dt = ASSIGN if grain == F.TAXID else ASSIGN_GI
    out = np.zeros(len(recs), dtype=dt)
    if recs:
        cols = np.array(recs, dtype=np.uint64).reshape(len(recs), len(dt.names))
        for k, f in enumerate(dt.names):
            out[f] = cols[:, k]
    return out


def ids(n_reads):
    """the read IDs of the sequences: lengths of 2 to 7 bytes, some with a ':' inside"""
    return [("q:%d" % k) if k % 7 == 3 else ("r%d" % k) for k in range(n_reads)]


def text_of(grain, recs, n_reads):
    names = ids(n_reads)
    return (A.text(recs, names) if grain == F.TAXID else GR.text(recs, names)).encode()


class Seen:
    """everything the observers of a fold return, for one state"""

    def __init__(self, grain, n_reads, recs):
        self.n_reads = n_reads
        self.count = len(recs)
        self.records = as_array(grain, recs).tobytes()
        self.report = F.report(recs)
        self.flags = F.flags(recs, n_reads)
        self.text = text_of(grain, recs, n_reads)

    def same(self, o):
        return o is not None and (self.n_reads, self.count, self.records) == (o.n_reads, o.count, o.records)


class FoldState:
    def __init__(self, grain):
        self.grain, self.n_reads, self.recs, self.taxa = grain, 0, [], set()
        # records the two arrays hold: Fold::stage_write of csrc/fold.hip restated -- max(2 * cap, wanted, FIRST_ALLOCATION) when a
        # result does not fit -- which lca.hip, pair.hip and dedup.hip call with the size of their result.  No observer returns the
        # capacity; test_lifecycle_cpu.py pins the rule to those source lines.
        self.cap = 0

        self._seen = None

    def put(self, n_reads, recs, taxa, room=None):
        """the fold becomes (n_reads, recs, taxa): an output of lca, pair or expand, or the result of a fold, which asks for
        room for both lists before equal keys are joined"""
        room = len(recs) if room is None else room
        if room > self.cap:
            self.cap = max(2 * self.cap, room, FIRST_ALLOCATION)
        self.n_reads, self.recs, self.taxa, self._seen = n_reads, recs, set(taxa), None

    def seen(self):
        if self._seen is None:
            self._seen = Seen(self.grain, self.n_reads, self.recs)
        return self._seen


def text_lines_tokens(lines):
    return sum(len(h.split(",")) for _, h in lines if h != "")


class FoldModel:
    """folds: {name: grain}.  apply(step) returns what the step must give: {"code": a refusal's error code} or
    {"result": ..., "seen": {handle: Seen}} for the handles the step touched."""

    def __init__(self, folds, taxonomy_text):
        self.f = {name: FoldState(g) for name, g in folds.items()}
        self.tx = LR.Taxonomy(taxonomy_text)
        self.map = None  # (read, rep) of the last take

    # ---- what the header refuses, and with which code ----
    def refusal(self, s):
        op = s["op"]
        f = self.f.get(s.get("h"))
        if op in ("lca", "pair"):
            out = self.f[s["out"]]
            if out is f or out.grain != F.TAXID:
                return E_ARG
        if op == "pair":
            if s["mode"] not in (PR.BOTH, PR.EITHER, PR.PROPER) or f.n_reads & 1 or (s["mode"] == PR.PROPER and f.grain != F.LONG):
                return E_ARG
            if s["mode"] == PR.EITHER and s["unpaired"] >= B31:
                return E_ARG
            if any(r[-1] >= B31 for r in f.recs):
                return E_ARG
        if op == "add_records":
            if not F.is_list(f.grain, s["records"]) or any(r[0] >= f.n_reads for r in s["records"]):
                return E_ARG
        if op == "add_text":
            try:
                TR.records(f.grain, s["lines"], f.n_reads)
            except TR.Format:
                return E_FORMAT
            except TR.Arg:
                return E_ARG
        if op == "format_text" and s["n_ids"] != f.n_reads:
            return E_ARG
        if op == "expand":
            src = self.f[s["src"]]
            if src is f or src.grain != f.grain or self.map is None:
                return E_ARG
            reps = {k for r, k in zip(*self.map) if r == k}
            if any(r[0] not in reps for r in src.recs):
                return E_ARG
        return None

    def apply(self, s):
        op = s["op"]
        if op == "refuse":
            code = self.refusal(s["call"])
            assert code is not None and code == s["code"], (s["why"], code)
            return {"code": code}
        assert self.refusal(s) is None, s["op"]
        f = self.f.get(s.get("h"))
        touched, result = [s["h"]] if "h" in s else [], None
        if op == "reset":
            f.put(s["n_reads"], [], ())
        elif op == "add_records":
            f.put(f.n_reads, F.fold(f.grain, f.recs, s["records"]), f.taxa | {r[1] for r in s["records"]},
                  room=(len(f.recs) + len(s["records"])) if s["records"] else 0)
        elif op == "add_text":
            recs = TR.records(f.grain, s["lines"], f.n_reads)
            result = (text_lines_tokens(s["lines"]), len(recs))
            f.put(f.n_reads, F.fold(f.grain, f.recs, recs), f.taxa | {r[1] for r in recs}, room=(len(f.recs) + len(recs)) if recs else 0)
        elif op == "lca":
            out = self.f[s["out"]]
            lcas = LR.per_read(self.tx, f.recs, s["slack"])
            rows = [(t, p, code, depth, direct, clade) for t, p, _, code, depth, direct, clade in LR.clade_rows(self.tx, lcas)]
            result = (rows, len(lcas))
            out.put(f.n_reads, lcas, {t for _, t, _ in lcas})
            touched = [s["out"], s["h"]]
        elif op == "pair":
            out = self.f[s["out"]]
            joined = PR.pair(s["mode"], f.recs, s["max_insert"], s["unpaired"])
            result = PR.stats(f.recs, f.n_reads, joined)
            out.put(f.n_reads // 2, joined, f.taxa)
            touched = [s["out"], s["h"]]
        elif op == "take":
            reads = D.read_codes(np.frombuffer(b"".join(s["reads"]), dtype=np.uint8), np.cumsum([0] + [len(r) for r in s["reads"]]))
            self.map = D.dupmap(reads)
            result = (self.map, len(D.representatives(reads)))
        elif op == "expand":
            src = self.f[s["src"]]
            f.put(src.n_reads, D.expand(src.recs, *self.map), src.taxa)
            touched = [s["h"], s["src"]]
        else:
            raise ValueError(op)
        return {"result": result, "seen": {h: self.f[h].seen() for h in touched},
                "cap": {h: self.f[h].cap for h in touched}}


def run_fold(folds, taxonomy_text, steps):
    m = FoldModel(folds, taxonomy_text)
    return [m.apply(s) for s in steps]


# ---- workspaces ------------------------------------------------------------------------------------------------------
# A batch is a list of reads (bytes).  A workspace's resident reads are kept as the letters of their codes ("ACGTN"): binning
# is a function of the codes, so the CPU oracle gives for them what it gives for the raw bytes.

OFF, WITH_HITS, ONLY = 0, 1, 2  # MTSV_MATCH_* and MTSV_ASSIGN_*
PARAM_SETS = {
    "default": {},
    "stress": dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5),
    "dense": dict(seed_size=10, seed_interval=3, max_hits=100000, tune_max_hits=30),
}
MAX_READ_LEN = 32767  # "this build verifies reads up to 32767"
COLLAPSE = {F.TAXID: A.collapse, F.LONG: GR.collapse_long, F.TAXID_GI: GR.collapse_taxid_gi}
HIT = np.dtype({"names": ["read", "tax_id", "gi", "edit", "strand", "offset"], "formats": ["<u8", "<u4", "<u4", "<u4", "u1", "<u8"],
                "offsets": [0, 8, 12, 16, 20, 24], "itemsize": 32})
FIELDS = ("read", "tax_id", "gi", "edit", "strand", "offset")
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


def letters(read):
    """a read as the letters of its normalised codes"""
    import chain_ref as CR
    return LETTERS[CR.normalise(np.frombuffer(read, dtype=np.uint8))].tobytes()


def batch_arrays(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if reads else np.zeros(0, np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return bases, off


def same_hits(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


class Oracles:
    """the CPU oracle of every database, its hits cached per (database, reads, parameter set)"""

    def __init__(self, dbs):
        from oracle import oracle as O
        self.O, self.ix, self.cache = O, {name: O.Index.build(entries) for name, entries in dbs.items()}, {}
        self.taxa = {name: sorted({e[0] for e in entries}) for name, entries in dbs.items()}

    def hits(self, db, reads, pname):
        key = (db, pname, hash(tuple(reads)), len(reads))
        if key not in self.cache:
            over = {("seed_gap" if k == "seed_interval" else k): v for k, v in PARAM_SETS[pname].items()}
            h, ctr = self.ix[db].bin_batch(*batch_arrays(reads), self.O.default_params(**over), threads=8)
            out = np.zeros(len(h), dtype=HIT)
            for f in FIELDS:
                out[f] = h[f]
            self.cache[key] = (out, (ctr["H"], ctr["n_cand"], ctr["n_sw"], ctr["W"]))
        return self.cache[key]


class Ws:
    def __init__(self, db):
        self.db = db
        self.reads, self.map, self.origin_n = None, None, 0     # the resident batch, its read map (None: the identity), the caller's n
        self.host = False                                        # the resident batch is a host batch's
        self.assign, self.grain, self.match, self.verify = OFF, F.TAXID, OFF, 0
        self.report_on, self.report, self.report_total = False, {}, 0
        self.last = None       # the last completed run: {"kind", "hits", "n", "presence", "counters"}; None after new reads came in
        # True: a run has completed since the flags / the assignments were switched on; False: none has, and the header says what
        # the observer returns; None: new reads came in since, and the header does not say
        self.flags_run = self.assign_run = False


class BatchSeen:
    """what the observers of a workspace must return in its state; None: the header does not say, nothing is asked"""

    def __init__(self, w):
        self.hits = self.stats = self.assign = self.text = self.flags = self.report = self.resident = None
        self.grain = w.grain
        if w.report_on:
            self.report = ({t: list(c) for t, c in w.report.items()}, w.report_total)
        if w.reads is not None and not w.host:
            codes = np.frombuffer(b"".join(w.reads), dtype=np.uint8)
            lut = np.zeros(256, dtype=np.uint8)
            lut[LETTERS] = np.arange(5, dtype=np.uint8)
            self.resident = (lut[codes].tobytes(), np.cumsum([0] + [len(r) for r in w.reads]).tolist(),
                             list(range(len(w.reads))) if w.map is None else list(w.map))
        if w.match != OFF and w.flags_run is False:
            self.flags = (np.zeros(0, dtype=bool), 0)            # "no run since the flags were switched on: *n_reads is 0"
        if w.assign != OFF and w.assign_run is False:
            self.assign = as_array(w.grain, []).tobytes()        # "no run since the assignments were switched on: *n is 0"
        if w.last is None:
            return
        hits, kind = w.last["hits"], w.last["kind"]
        gathered = w.match != ONLY
        self.hits = hits if (gathered and w.assign != ONLY) else hits[:0]
        self.stats = {"n_reads": w.last["n"], "n_hits": len(hits) if gathered else 0}
        if kind == "merged":
            self.stats.update(n_seed_hits=0, n_candidates=0, n_verified=0, window_bytes=0)
        elif w.last["counters"] is not None:
            self.stats.update(zip(("n_seed_hits", "n_candidates", "n_verified", "window_bytes"), w.last["counters"]))
        if w.match != OFF and w.flags_run is True:
            self.flags = (w.last["presence"], int(w.last["presence"].sum()))
        if w.assign != OFF and w.assign_run is True:
            recs = COLLAPSE[w.grain](hits)
            self.assign = as_array(w.grain, recs).tobytes()
            if kind != "host":
                self.text = text_of(w.grain, recs, w.origin_n)
                self.text_n = w.origin_n


class BatchModel:
    """workspaces: {name: database}; dbs: {database: entries}; one fold "fold" of the grain fold_grain that takes runs"""

    def __init__(self, workspaces, dbs, fold_grain, oracles=None):
        self.orc = oracles or Oracles(dbs)
        self.w = {name: Ws(db) for name, db in workspaces.items()}
        self.fold = FoldState(fold_grain)
        self.dupmap = None

    def refusal(self, s):
        op, w = s["op"], self.w.get(s.get("w"))
        src = self.w.get(s.get("src"))
        if op == "set_assignment_grain" and w.assign != OFF:
            return E_ARG
        if op == "set_assignments" and s["mode"] != OFF and w.match == ONLY:
            return E_ARG
        if op == "set_match_flags" and s["mode"] == ONLY and (w.report_on or w.assign != OFF):
            return E_ARG
        if op == "set_taxa_report" and s["on"] and w.match == ONLY:
            return E_ARG
        if op == "download_assignments" and (w.assign == OFF or s["wide"] != (w.grain != F.TAXID)):
            return E_ARG
        if op == "taxa_report" and not w.report_on:
            return E_ARG
        if op == "match_flags" and w.match == OFF:
            return E_ARG
        if op == "format_text" and (w.assign == OFF or w.last is None or w.last["kind"] == "host"):
            return E_ARG
        if op == "add_run" and (src.assign == OFF or src.grain != self.fold.grain or src.last is None or src.last["kind"] == "host"):
            return E_ARG
        if op == "run":
            if any(len(r) > MAX_READ_LEN for r in w.reads):
                return E_LIMIT
        if op in ("run_host", "run_host_parts"):
            reads = s["reads"] if op == "run_host" else [r for p in s["parts"] for r in p]
            if any(len(r) > MAX_READ_LEN for r in reads):
                return E_LIMIT
        if op == "take_reads":
            if src is w or src.match == OFF or src.last is None or src.last["kind"] == "merged" or src.flags_run is not True or src.reads is None:
                return E_ARG
        if op in ("copy_reads", "take_unique") and (src is w or src.reads is None):
            return E_ARG
        if op == "merge_runs":
            srcs = [self.w[x] for x in s["srcs"]]
            if w in srcs or w.match == ONLY or any(x.last is None or x.last["kind"] != "resident" or x.match == ONLY for x in srcs):
                return E_ARG
            if len({tuple(len(r) for r in x.reads) for x in srcs}) != 1 or len({x.map is None for x in srcs}) != 1:
                return E_ARG
        return None

    def ran(self, w, kind, hits, n, presence, counters):
        """a completed run: the results of the run before are replaced, the report takes the reads"""
        w.last = {"kind": kind, "hits": hits, "n": n, "presence": presence, "counters": counters}
        w.flags_run, w.assign_run = w.match != OFF, w.assign != OFF
        if w.report_on:
            import taxa_report_ref as R
            stats, total = R.classify_hits(hits)
            for t, c in stats.items():
                row = w.report.setdefault(t, [0, 0, 0, 0])
                for k in range(4):
                    row[k] += c[k]
            w.report_total += total

    def run_on(self, w, reads, pname, kind, read_map):
        hits, counters = self.orc.hits(w.db, reads, pname)
        presence = np.zeros(len(reads), dtype=bool)
        presence[hits["read"].astype(np.int64)] = True
        if read_map is not None:
            hits = hits.copy()
            hits["read"] = np.asarray(read_map, dtype=np.uint64)[hits["read"].astype(np.int64)] if len(hits) else hits["read"]
        # (the work counters where tests/fuzz_parity.py compares them: an uploaded batch, the reference's order, no cut-off)
        plain = w.verify == 0 and "max_assignments" not in PARAM_SETS[pname] and w.match != ONLY and kind == "resident" and read_map is None
        self.ran(w, kind, hits, len(reads), presence, counters if plain else None)

    def new_reads(self, w, reads, read_map, origin_n, host=False):
        w.reads, w.map, w.origin_n, w.host, w.last = reads, read_map, origin_n, host, None
        w.flags_run = None if w.match != OFF else False
        w.assign_run = None if w.assign != OFF else False

    def apply(self, s):
        op = s["op"]
        if op == "refuse":
            code = self.refusal(s["call"])
            assert code is not None and code == s["code"], (s["why"], code)
            # every handle must give afterwards what it gave before: what the model holds (a host batch's hits are handed out once)
            seen = {name: BatchSeen(x) for name, x in self.w.items()}
            for name, x in seen.items():
                if self.w[name].last is not None and self.w[name].last["kind"] == "host":
                    x.hits = None
            return {"code": code, "seen": seen, "fold": self.fold.seen()}
        assert self.refusal(s) is None, op
        w, src, result, touched = self.w.get(s.get("w")), self.w.get(s.get("src")), None, [s["w"]] if "w" in s else []
        fold_seen = None
        if op == "upload":
            self.new_reads(w, [letters(r) for r in s["reads"]], None, len(s["reads"]))
        elif op == "run":
            self.run_on(w, w.reads, s["params"], "resident", w.map)
        elif op in ("run_host", "run_host_parts"):
            reads = [letters(r) for r in (s["reads"] if op == "run_host" else [r for p in s["parts"] for r in p])]
            self.new_reads(w, reads, None, len(reads), host=True)
            self.run_on(w, reads, s["params"], "host", None)
        elif op == "set_verify_mode":
            w.verify = s["mode"]
        elif op == "set_assignments":
            if s["mode"] != OFF and w.assign == OFF:
                w.assign_run = False
            w.assign = s["mode"]
        elif op == "set_assignment_grain":
            w.grain = s["grain"]
        elif op == "set_match_flags":
            if s["mode"] != OFF and w.match == OFF:
                w.flags_run = False
            w.match = s["mode"]
        elif op == "set_taxa_report":
            w.report_on = bool(s["on"])
        elif op == "taxa_report":
            result = ({t: list(c) for t, c in w.report.items()}, w.report_total)
            if s["reset"]:
                w.report, w.report_total = {}, 0
        elif op == "take_reads":
            keep = src.last["presence"] if s["keep"] else ~src.last["presence"]
            idx = np.nonzero(keep)[0].tolist()
            reads = [src.reads[j] for j in idx]
            self.new_reads(w, reads, idx if src.map is None else [src.map[j] for j in idx], src.origin_n)
            result = (len(reads), sum(len(r) for r in reads))
        elif op == "copy_reads":
            self.new_reads(w, list(src.reads), None if src.map is None else list(src.map), src.origin_n)
        elif op == "take_unique":
            read, rep = D.dupmap(src.reads, src.map)
            idx = D.representatives(src.reads)
            reads = [src.reads[j] for j in idx]
            self.new_reads(w, reads, [read[j] for j in idx], src.origin_n)
            self.dupmap = (read, rep)
            result = (len(reads), sum(len(r) for r in reads), read, rep)
        elif op == "merge_runs":
            import chunk_merge_ref as CM
            srcs = [self.w[x] for x in s["srcs"]]
            merged = CM.merge_hits([x.last["hits"] for x in srcs])
            presence = np.logical_or.reduce([x.last["presence"] for x in srcs])
            w.origin_n = srcs[0].origin_n
            self.ran(w, "merged", merged, srcs[0].last["n"], presence, None)
        elif op == "fold_reset":
            self.fold.put(s["n_reads"], [], ())
            touched = []
        elif op == "add_run":
            recs = COLLAPSE[self.fold.grain](src.last["hits"])
            taxa = {r[1] for r in recs} if src.last["kind"] == "merged" else set(self.orc.taxa[src.db])
            self.fold.put(self.fold.n_reads, F.fold(self.fold.grain, self.fold.recs, recs), self.fold.taxa | taxa,
                          room=(len(self.fold.recs) + len(recs)) if recs else 0)
            touched = []
        else:
            raise ValueError(op)
        if op in ("fold_reset", "add_run"):
            fold_seen = self.fold.seen()
        seen = {name: BatchSeen(self.w[name]) for name in touched}
        if op not in ("run_host", "run_host_parts"):
            for x in seen.values():      # (a host batch's hits are handed out once: only the step that ran it asks for them)
                if self.w[s["w"]].last is not None and self.w[s["w"]].last["kind"] == "host":
                    x.hits = None
        return {"result": result, "seen": seen, "fold": fold_seen}
