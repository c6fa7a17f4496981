"""-m gpu sequence tests: a seeded list of operations (lifecycle_cases.py) replayed on a few handles that live through the whole
list, every observable result after every step compared with the Python model (lifecycle_model.py).

The per-feature tests make a handle, call it once or a few times and close it.  These tests pin down what only history can
break: a scratch array that is cleared only where it grows, the tail of a large call showing through a small one, a counter
that is not zeroed again, a refused call that leaves something behind.  Expected values never come from the device or from an
earlier device result: the model derives them from the restatements and the CPU oracle.  Every comparison is exact; a
sequence stops at its first mismatch and names the seed, the step and the three steps before it."""
import numpy as np
import pytest

import helpers
import lifecycle_cases as LC
import lifecycle_model as LM
import mtsv_tools_amd as M
import parse_ref as TR
import taxa_report_ref as R

pytestmark = pytest.mark.gpu

SMALL = {"MTSV_FOLD_TILE": "2", "MTSV_TEXT_TILE": "2", "MTSV_PARSE_TILE": "64", "MTSV_LCA_TILE": "64", "MTSV_PAIR_TILE": "64",
         "MTSV_PAIR_LANE_MAX": "3", "MTSV_FAN_TILE": "64"}
SETTINGS = {"defaults": {}, "small": SMALL}
_expected = {}
_id_tables = {}


def configure(monkeypatch, setting):
    """the tile and tier settings are read when a handle is created: set before the handles are made"""
    for name in SMALL:
        if name in SETTINGS[setting]:
            monkeypatch.setenv(name, SETTINGS[setting][name])
        else:
            monkeypatch.delenv(name, raising=False)


def expected_fold(seed):
    """the model's answers, computed once per seed and never changed"""
    if seed not in _expected:
        folds, steps = LC.sequence("fold", seed)
        _expected[seed] = LM.run_fold(folds, open(LC.TAXONOMY).read(), steps)
    return _expected[seed]


def id_table(n_reads):
    if n_reads not in _id_tables:
        names = LM.ids(n_reads)
        blob = b"".join(i.encode() + b"\0" for i in names)
        off = np.zeros(n_reads + 1, dtype=np.uint64)
        np.cumsum([len(i) + 1 for i in names], out=off[1:])
        _id_tables[n_reads] = (blob, off)
    return _id_tables[n_reads]


def raw(fold):
    return (fold.download() if fold.grain == M.GRAIN_TAXID else fold.download_gi()).tobytes()


def check_seen(name, fold, seen):
    """every observer of a fold against the model's state"""
    assert fold.count() == seen.count, (name, "count", fold.count(), seen.count)
    got = raw(fold)
    if got != seen.records:
        size = 16 if fold.grain == M.GRAIN_TAXID else 24
        at = next((k for k in range(min(len(got), len(seen.records)) // size) if got[k * size:(k + 1) * size] != seen.records[k * size:(k + 1) * size]), None)
        raise AssertionError((name, "records", len(got) // size, len(seen.records) // size, "first difference at record", at))
    rows, total, _ = fold.taxa_report()
    assert rows["tax_id"].tolist() == sorted(set(rows["tax_id"].tolist())), (name, "report rows do not ascend")
    assert (R.rows_dict(rows), total) == seen.report, (name, "taxa report")
    flags, matched = fold.match_flags()
    assert len(flags) == seen.n_reads and np.array_equal(flags, seen.flags) and matched == int(seen.flags.sum()), (name, "match flags", matched)
    text, _ = fold.format_text(id_table(seen.n_reads))
    assert text == seen.text, (name, "text", len(text), len(seen.text))


class FoldRig:
    """the handles of a fold sequence"""

    def __init__(self, folds, ix):
        self.f = {name: M.Fold(0, grain) for name, grain in folds.items()}
        self.map = M.DupMap(0)
        self.tx = M.Taxonomy(LC.TAXONOMY)
        self.intake = M.Batch(ix, 0, 4200, 4200 * 16, lanes=1)
        self.unique = M.Batch(ix, 0, 4200, 4200 * 16, lanes=1)

    def close(self):
        for x in (*self.f.values(), self.map, self.tx, self.intake, self.unique):
            x.close()

    def state(self):
        read, rep, n_unique = self.map.download()
        return [(f.count(), raw(f)) for f in self.f.values()], read.tobytes(), rep.tobytes(), n_unique

    def call(self, s):
        """one step on the device; returns what the model calls its result"""
        op = s["op"]
        f = self.f.get(s.get("h"))
        if op == "reset":
            f.reset(s["n_reads"])
        elif op == "add_records":
            f.add_records(LM.as_array(f.grain, s["records"]))
        elif op == "add_text":
            return f.add_text(*TR.arrays(s["lines"]))[:2]
        elif op == "lca":
            rows, total, _ = f.lca(self.tx, s["slack"], out=self.f[s["out"]])
            return [tuple(int(r[c]) for c in ("tax_id", "parent_tax_id", "rank", "depth", "direct", "clade")) for r in rows], total
        elif op == "pair":
            return f.pair(s["mode"], s["max_insert"], s["unpaired"], out=self.f[s["out"]])[0]
        elif op == "take":
            self.intake.upload(*helpers.reads_to_batch(s["reads"]))
            n_unique = self.unique.take_unique(self.intake, self.map)[0]
            read, rep, n2 = self.map.download()
            assert n2 == n_unique
            return (read.tolist(), rep.tolist()), n_unique
        elif op == "expand":
            f.expand(self.f[s["src"]], self.map)
        elif op == "format_text":
            f.format_text(id_table(s["n_ids"]))
        else:
            raise ValueError(op)
        return None

    def step(self, s, want):
        if s["op"] == "refuse":
            before = self.state()
            with pytest.raises(M.MtsvError) as e:
                self.call(s["call"])
            assert e.value.code == want["code"], (s["why"], str(e.value))
            assert self.state() == before, (s["why"], "a refused call changed a handle")
            return
        got = self.call(s)
        assert got == want["result"], ("result", got if s["op"] != "take" else "(the map)", want["result"] if s["op"] != "take" else "")
        for name, seen in want["seen"].items():
            check_seen(name, self.f[name], seen)


def replay(kind, seed, steps, expected, rig):
    assert len(steps) == len(expected)
    for k, (s, want) in enumerate(zip(steps, expected)):
        try:
            rig.step(s, want)
        except (AssertionError, M.MtsvError) as e:
            last = "\n".join(f"  step {j}: {LC.brief(steps[j])}" for j in range(max(0, k - 3), k + 1))
            raise AssertionError(f"{kind} sequence, seed {seed}: step {k} of {len(steps)} failed: {e}\n{last}") from e


@pytest.fixture(scope="module")
def tiny_ix():
    ix = M.MGIndex.synth(seed=31, n_taxa=4, gis_per_taxon=1, seq_len=3000)
    ix.to_device(0)
    yield ix
    ix.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("seed", LC.FOLD_SEEDS)
def test_fold_sequences(seed, setting, tiny_ix, monkeypatch):
    configure(monkeypatch, setting)
    folds, steps = LC.sequence("fold", seed)
    expected = expected_fold(seed)
    rig = FoldRig(folds, tiny_ix)
    try:
        replay("fold", seed, steps, expected, rig)
    finally:
        rig.close()


# ---- workspaces ----

def check_ws(name, ws, seen):
    """every observer of a workspace the header defines in the state the model is in"""
    if seen.resident is not None:
        codes, off = ws.download_reads()
        assert (codes.tobytes(), off.tolist()) == seen.resident[:2], (name, "resident reads", len(off) - 1, len(seen.resident[1]) - 1)
        assert ws.read_map().tolist() == seen.resident[2], (name, "read map")
    if seen.hits is not None:
        got = ws.download()
        assert len(got) == len(seen.hits), (name, "hits", len(got), len(seen.hits))
        helpers.assert_same_hits(got, seen.hits)
    if seen.stats is not None:
        st = ws.stats()
        assert {k: st[k] for k in seen.stats} == seen.stats, (name, "stats", {k: st[k] for k in seen.stats}, seen.stats)
    if seen.flags is not None:
        flags, matched = ws.match_flags()
        assert len(flags) == len(seen.flags[0]) and np.array_equal(flags, seen.flags[0]) and matched == seen.flags[1], (name, "match flags", len(flags), matched, seen.flags[1])
    if seen.assign is not None:
        got = (ws.download_assignments() if seen.grain == M.GRAIN_TAXID else ws.download_assignments_gi())[0].tobytes()
        assert got == seen.assign, (name, "assignments", len(got), len(seen.assign))
    if seen.text is not None:
        assert ws.format_text(id_table(seen.text_n))[0] == seen.text, (name, "text")
    if seen.report is not None:
        rows, total, _ = ws.taxa_report(False)
        assert (R.rows_dict(rows), total) == seen.report, (name, "taxa report", total, seen.report[1])


class BatchRig:
    """the handles of a workspace sequence: they live through the whole list"""

    def __init__(self, info, indexes, lanes):
        self.w = {name: M.Batch(indexes[db], 0, LC.MAX_READS, LC.MAX_BASES, lanes=lanes) for name, db in info["workspaces"].items()}
        self.fold = M.Fold(0, info["fold_grain"])
        self.map = M.DupMap(0)

    def close(self):
        for x in (*self.w.values(), self.fold, self.map):
            x.close()

    def call(self, s):
        op, ws = s["op"], self.w.get(s.get("w"))
        src = self.w.get(s.get("src"))
        if op == "upload":
            ws.upload(*LM.batch_arrays(s["reads"]))
        elif op == "run":
            ws.run(M.default_params(**LM.PARAM_SETS[s["params"]]))
        elif op == "run_host":
            ws.run_host(*LM.batch_arrays(s["reads"]), M.default_params(**LM.PARAM_SETS[s["params"]]))
        elif op == "run_host_parts":
            ws.run_host_parts([LM.batch_arrays(p) for p in s["parts"]], M.default_params(**LM.PARAM_SETS[s["params"]]))
        elif op == "set_verify_mode":
            ws.set_verify_mode(s["mode"])
        elif op == "set_assignments":
            ws.set_assignments(s["mode"])
        elif op == "set_assignment_grain":
            ws.set_assignment_grain(s["grain"])
        elif op == "set_match_flags":
            ws.set_match_flags(s["mode"])
        elif op == "set_taxa_report":
            ws.set_taxa_report(s["on"])
        elif op == "taxa_report":
            rows, total, _ = ws.taxa_report(bool(s["reset"]))
            return R.rows_dict(rows), total
        elif op == "take_reads":
            return ws.take_reads(src, s["keep"])[:2]
        elif op == "copy_reads":
            ws.copy_reads(src)
        elif op == "take_unique":
            n_unique, bases_kept, _ = ws.take_unique(src, self.map)
            read, rep, n2 = self.map.download()
            assert n2 == n_unique
            return n_unique, bases_kept, read.tolist(), rep.tolist()
        elif op == "merge_runs":
            ws.merge_runs([self.w[x] for x in s["srcs"]])
        elif op == "fold_reset":
            self.fold.reset(s["n_reads"])
        elif op == "add_run":
            self.fold.add_run(src)
        elif op == "download_assignments":
            ws.download_assignments_gi() if s["wide"] else ws.download_assignments()
        elif op == "format_text":
            ws.format_text(id_table(s["n_ids"]))
        else:
            raise ValueError(op)
        return None

    def step(self, s, want):
        if s["op"] == "refuse":
            with pytest.raises(M.MtsvError) as e:
                self.call(s["call"])
            assert e.value.code == want["code"] and s["says"] in str(e.value), (s["why"], str(e.value))
        else:
            got = self.call(s)
            assert got == want["result"], ("result", got, want["result"])
        # the handles the step touched; after a refusal every handle, which must give what it gave before the call
        for name, seen in want["seen"].items():
            check_ws(name, self.w[name], seen)
        if want["fold"] is not None:
            check_seen("fold", self.fold, want["fold"])


@pytest.fixture(scope="module")
def indexes():
    out = {}
    for name, (entries, _, _) in LC.databases().items():
        out[name] = M.MGIndex.build(entries, threads=4)
        out[name].to_device(0)
    yield out
    for ix in out.values():
        ix.close()


@pytest.mark.parametrize("lanes", [1, 0], ids=["one_lane", "default_lanes"])
@pytest.mark.parametrize("seed", LC.BATCH_SEEDS)
def test_batch_sequences(seed, lanes, indexes):
    info, steps = LC.sequence("batch", seed)
    expected = LC.expected_batch(seed)
    rig = BatchRig(info, indexes, lanes)
    try:
        replay("batch", seed, steps, expected, rig)
    finally:
        rig.close()
