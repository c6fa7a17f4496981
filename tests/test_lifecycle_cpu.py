"""No GPU: the reference side of the sequence tests (lifecycle_cases.py, lifecycle_model.py) meets the conditions the GPU
tests rest on -- the same seed gives the same steps, every call that owns scratch memory meets the histories that could break
it (the coverage table: a condition on the generator, asserted, not measured), the model equals the restatements it wraps,
and no step is trivial."""
import copy

import numpy as np
import pytest

import dedup_ref as D
import fold_ref as F
import lca_ref as LR
import lifecycle_cases as LC
import lifecycle_model as LM
import pair_ref as PR
import parse_ref as TR

TAXONOMY_TEXT = open(LC.TAXONOMY).read()
# the calls that own scratch memory (or, for the observers, read state that a larger call left): the handle that owns it
OWNERS = ("lca", "pair_both", "pair_either", "pair_proper", "format_text", "add_text", "expand", "taxa_report", "match_flags", "add_records")
OBSERVERS = ("format_text", "taxa_report", "match_flags")
TILE = 1024  # the largest tile of the tiled passes: fewer tiles at this size is fewer at every smaller one
_runs = {}


def words(n_reads):
    return (n_reads + 63) // 64


def tiles(n):
    return (n + TILE - 1) // TILE


def run(seed):
    """(steps, expectations, calls): calls is {owner op: {handle: [(step, records, reads)]}} in step order, the size of what
    each call worked on; outputs is [(step, op, result length, capacity of out before)]"""
    if seed not in _runs:
        folds, steps = LC.sequence("fold", seed)
        m = LM.FoldModel(folds, TAXONOMY_TEXT)
        expected, calls, outputs = [], {op: {} for op in OWNERS}, []

        def note(op, handle, k, records, reads):
            calls[op].setdefault(handle, []).append((k, records, reads))

        for k, s in enumerate(steps):
            op = s["op"]
            f = m.f.get(s.get("h"))
            if op == "lca":
                note("lca", s["h"], k, len(f.recs), f.n_reads)
            elif op == "pair":
                note("pair_" + {PR.BOTH: "both", PR.EITHER: "either", PR.PROPER: "proper"}[s["mode"]], s["h"], k, len(f.recs), f.n_reads)
            elif op == "add_records":
                note("add_records", s["h"], k, len(s["records"]), f.n_reads)
            elif op == "add_text":
                note("add_text", s["h"], k, len(TR.records(f.grain, s["lines"], f.n_reads)), f.n_reads)
            elif op == "expand":
                note("expand", "map", k, len(m.f[s["src"]].recs), len(m.map[0]))
            cap_before = m.f["out"].cap
            e = m.apply(s)
            expected.append(e)
            if op in ("lca", "pair"):
                outputs.append((k, op, len(m.f["out"].recs), cap_before))
            for h in e.get("seen", {}):
                for o in OBSERVERS:
                    note(o, h, k, len(m.f[h].recs), m.f[h].n_reads)
        _runs[seed] = (steps, expected, calls, outputs)
    return _runs[seed]


def test_the_same_seed_gives_the_same_steps():
    for seed in LC.FOLD_SEEDS:
        a = copy.deepcopy(LC.fold_sequence(seed))
        assert a == LC.fold_sequence(seed) == LC.sequence("fold", seed)
    assert LC.fold_sequence(1)[1] != LC.fold_sequence(2)[1]


def test_the_gpu_file_uses_these_seeds():
    src = open(LC.__file__.replace("lifecycle_cases.py", "test_lifecycle.py")).read()
    assert '@pytest.mark.parametrize("seed", LC.FOLD_SEEDS)' in src


def smaller_after_larger(history):
    """a call on a larger input and a later one on a smaller, non-empty one: fewer records, reads, tiles and flag words, the last
    flag word not full"""
    return any(r0 > r1 > 0 and n0 > n1 and tiles(r0) > tiles(r1) and words(n0) > words(n1) and n1 % 64
               for i, (_, r0, n0) in enumerate(history) for _, r1, n1 in history[i + 1:])


def empty_between(history):
    sizes = [r for _, r, _ in history]
    return any(sizes[j] == 0 and any(sizes[:j]) and any(sizes[j + 1:]) for j in range(len(sizes)))


@pytest.mark.parametrize("seed", LC.FOLD_SEEDS)
def test_coverage_table_of_the_fold_sequences(seed):
    steps, _, calls, outputs = run(seed)
    table = {}
    for op in OWNERS:
        rows = {h: (smaller_after_larger(hist), empty_between(hist)) for h, hist in calls[op].items()}
        table[op] = rows
        assert any(a and b for a, b in rows.values()), (op, rows)                       # 1, 2 and 4, on one handle
    # 3. the output fold of lca and of pair: a result longer than its capacity, a shorter one, an empty one, one that is not
    for op in ("lca", "pair"):
        lens = [(n, cap) for _, o, n, cap in outputs if o == op]
        grew = [j for j, (n, cap) in enumerate(lens) if n > cap > 0]
        assert grew, (op, lens)
        j = grew[0]
        shorter = next((k for k in range(j + 1, len(lens)) if 0 < lens[k][0] < lens[j][0]), None)
        assert shorter is not None, op
        empty = next((k for k in range(shorter + 1, len(lens)) if lens[k][0] == 0), None)
        assert empty is not None, op
        assert any(n > 0 for n, _ in lens[empty + 1:]), op
    # the ladder: every rung is the size of some list or the number of some fold's reads
    sizes = {len(s["records"]) for s in steps if s["op"] == "add_records"} | {s["n_reads"] for s in steps if s["op"] == "reset"}
    sizes |= {len(s["reads"]) for s in steps if s["op"] == "take"}
    assert {0, 1, 4097, 140004} <= sizes and sizes & {63, 64, 65} and sizes & {1023, 1025} and sizes & {65535, 65537}
    assert sum(1 for s in steps if s["op"] in ("add_records", "add_text") and len(s.get("records", s.get("lines"))) > 65536) <= 2
    # every refusal of the list
    assert {s["why"] for s in steps if s["op"] == "refuse"} == {
        "out of a wide grain", "out is the fold itself", "an odd n_reads", "a record with an edit of 2^31", "keys that do not ascend",
        "an ID table of another length", "a malformed token"}


def test_both_sides_of_the_edges_over_the_seeds():
    sizes = set()
    for seed in LC.FOLD_SEEDS:
        steps = run(seed)[0]
        sizes |= {len(s["records"]) for s in steps if s["op"] == "add_records"} | {s["n_reads"] for s in steps if s["op"] == "reset"}
    assert {63, 64, 65, 1023, 1025, 65535, 65537} <= sizes


@pytest.mark.parametrize("seed", LC.FOLD_SEEDS)
def test_no_step_is_trivial(seed):
    steps, expected, _, _ = run(seed)
    last = {}
    for k, (s, e) in enumerate(zip(steps, expected)):
        if s["op"] == "refuse":
            continue
        work = {"add_records": lambda: len(s["records"]), "add_text": lambda: e["result"][1], "lca": lambda: e["seen"][s["h"]].count,
                "pair": lambda: e["seen"][s["h"]].count, "expand": lambda: e["seen"][s["src"]].count, "take": lambda: 1, "reset": lambda: 0}[s["op"]]()
        if s["op"] == "take":
            assert 1 < e["result"][1] < len(s["reads"])                                 # some reads are copies, not all
            continue
        target = s.get("out", s.get("h"))
        seen = e["seen"][target]
        if work:
            assert seen.count > 0, (k, LC.brief(s))
            assert not seen.same(last.get(target)), (k, LC.brief(s))
            if s["op"] in ("add_records", "add_text"):
                assert 0 < int(seen.flags.sum()) and seen.text
        last[target] = seen


# ---- the model against the restatements it wraps ----

def test_the_fold_model_equals_the_restatements_on_hand_made_sequences():
    for grain in (F.TAXID, F.TAXID_GI, F.LONG):
        wide = [(0, 9606, 1, 10, 2), (1, 9606, 1, 40, 1), (1, 9598, 2, 7, 0), (2, 9598, 1, 5, 3), (5, 9606, 1, 1, 1)]
        more = [(0, 9606, 1, 10, 1), (3, 9597, 1, 50, 4), (5, 9606, 1, 1, 6)]
        cut = (lambda r: (r[0], r[1], r[4])) if grain == F.TAXID else (lambda r: r)
        a, b = F.fold(grain, [], [cut(r) for r in wide]), F.fold(grain, [], [cut(r) for r in more])
        lines = [(4, "9601-1-3=2,9601-1-3=1"), (5, "")]
        steps = [{"op": "reset", "h": "f", "n_reads": 6}, {"op": "add_records", "h": "f", "records": a}, {"op": "add_text", "h": "f", "lines": lines},
                 {"op": "add_records", "h": "f", "records": b}, {"op": "lca", "h": "f", "slack": 0, "out": "o"},
                 {"op": "pair", "h": "f", "mode": PR.EITHER, "max_insert": 0, "unpaired": 2, "out": "o"}]
        m = LM.FoldModel({"f": grain, "o": F.TAXID}, TAXONOMY_TEXT)
        out = [m.apply(s) for s in steps]
        final = F.fold_all(grain, [a, TR.records(grain, lines, 6), b])
        assert m.f["f"].recs == final and out[3]["seen"]["f"].records == LM.as_array(grain, final).tobytes()
        assert out[2]["result"] == (2, 1)
        tx = LR.Taxonomy(TAXONOMY_TEXT)
        assert out[4]["seen"]["o"].records == LM.as_array(F.TAXID, LR.per_read(tx, final, 0)).tobytes() and out[4]["result"][1] == 6
        assert out[5]["seen"]["o"].records == LM.as_array(F.TAXID, PR.pair(PR.EITHER, final, 0, 2)).tobytes()
        assert out[5]["seen"]["o"].n_reads == 3 and out[5]["seen"]["f"].records == out[3]["seen"]["f"].records
        # a reset forgets, and a refusal changes nothing
        assert m.apply({"op": "refuse", "why": "odd", "code": LM.E_ARG, "call": {"op": "add_records", "h": "f", "records": a[::-1]}}) == {"code": LM.E_ARG}
        assert m.f["f"].recs == final
        assert m.apply({"op": "reset", "h": "f", "n_reads": 2})["seen"]["f"].count == 0 and m.f["f"].taxa == set()


def test_the_fold_model_expands_as_the_restatement_does():
    reads = [b"ACGTACGTAC", b"acgtacgtac", b"TTTTACGTAC", b"ACGTACGTAC", b"TTTTACGTAC", b"ACGTACGTA"]
    recs = [(0, 5, 1), (0, 7, 0), (2, 5, 3), (5, 9, 9)]
    m = LM.FoldModel({"rep": F.TAXID, "dst": F.TAXID}, TAXONOMY_TEXT)
    steps = [{"op": "take", "reads": reads}, {"op": "reset", "h": "rep", "n_reads": 6}, {"op": "add_records", "h": "rep", "records": recs},
             {"op": "expand", "h": "dst", "src": "rep"}]
    out = [m.apply(s) for s in steps]
    assert out[0]["result"] == (([0, 1, 2, 3, 4, 5], [0, 0, 2, 0, 2, 5]), 3)
    assert m.f["dst"].recs == D.expand(recs, *out[0]["result"][0]) == [(0, 5, 1), (0, 7, 0), (1, 5, 1), (1, 7, 0), (2, 5, 3), (3, 5, 1), (3, 7, 0), (4, 5, 3), (5, 9, 9)]
    assert m.f["dst"].n_reads == 6
    # records of a read that is no representative: refused
    assert m.refusal({"op": "add_records", "h": "rep", "records": [(1, 5, 1)]}) is None
    m.apply({"op": "add_records", "h": "rep", "records": [(1, 5, 1)]})
    assert m.refusal({"op": "expand", "h": "dst", "src": "rep"}) == LM.E_ARG


def test_the_capacity_the_model_keeps_is_the_accumulators_growth_rule():
    # coverage condition 3 ("a result longer than its capacity") is asserted against FoldState.cap, the model's restatement of
    # Fold::stage_write (fold.hip), which lca.hip, pair.hip and dedup.hip call with the size of their result: the rule is
    # pinned to the source here, so that a change of the library's rule shows up as a failure and not as a silent loss of coverage
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mtsv_tools_amd", "csrc")
    text = re.sub(r"\s+", " ", open(os.path.join(csrc, "fold.hip")).read())
    assert "if (n_records <= cap && d_rec[0].p)" in text
    assert "std::max<uint64_t>(std::max<uint64_t>(2 * cap, n_records), 1ull << 16)" in text
    for name, call in (("lca.hip", "out->stage_write(R,"), ("pair.hip", "out->stage_write(total,"), ("dedup.hip", "dst.stage_write(total,")):
        assert call in open(os.path.join(csrc, name)).read(), name
    s = LM.FoldState(F.TAXID)
    s.put(4, [(0, 1, 1)], ())
    assert s.cap == 65536
    s.put(4, [(0, 1, 1)] * 3, (), room=65537)
    assert s.cap == 131072
    s.put(4, [], (), room=0)
    assert s.cap == 131072
    s.put(4, [(0, 1, 1)], (), room=300000)
    assert s.cap == 300000


# ---- workspaces ----

BATCH_OWNERS = ("run", "run_host", "take_reads", "take_unique", "merge_runs", "collapse", "flags", "report")


def batch_run(seed):
    """(steps, expectations, {owner: {handle: [(step, reads, hits or records)]}})"""
    info, steps = LC.sequence("batch", seed)
    expected = LC.expected_batch(seed)
    calls = {op: {} for op in BATCH_OWNERS}
    for k, (s, e) in enumerate(zip(steps, expected)):
        op = s["op"]
        if op == "refuse":
            continue
        seen = e["seen"].get(s.get("w"))
        if op in ("run", "run_host", "run_host_parts", "merge_runs"):
            owner = "run_host" if op == "run_host_parts" else op
            n = seen.stats["n_reads"]
            calls[owner].setdefault(s["w"], []).append((k, n, seen.stats["n_hits"]))
            if seen.assign is not None:
                calls["collapse"].setdefault((s["w"], seen.grain), []).append((k, n, len(seen.assign)))
            if seen.flags is not None:
                calls["flags"].setdefault(s["w"], []).append((k, n, seen.flags[1]))
            if seen.report is not None:
                calls["report"].setdefault(s["w"], []).append((k, n, seen.stats["n_hits"]))
        elif op in ("take_reads", "take_unique"):
            calls[op].setdefault(s["w"], []).append((k, len(seen.resident[1]) - 1, e["result"][0]))
    return steps, expected, calls, info


def test_the_same_seed_gives_the_same_batch_steps():
    steps = LC.sequence("batch", 1)[1]
    assert LC.batch_sequence(1)[1] == steps and LC.batch_sequence(2)[1] != steps
    src = open(LC.__file__.replace("lifecycle_cases.py", "test_lifecycle.py")).read()
    assert '@pytest.mark.parametrize("seed", LC.BATCH_SEEDS)' in src


def shrinks(history):
    """a call on more reads with more results, and a later one on fewer reads with fewer results, of which there are some; the
    flag words fewer too"""
    return any(h0 > h1 > 0 and n0 > n1 and words(n0) > words(n1) for i, (_, n0, h0) in enumerate(history) for _, n1, h1 in history[i + 1:])


def empty_among(history):
    sizes = [h for _, _, h in history]
    return any(sizes[j] == 0 and any(sizes[:j]) and any(sizes[j + 1:]) for j in range(len(sizes)))


@pytest.mark.parametrize("seed", LC.BATCH_SEEDS)
def test_coverage_table_of_the_batch_sequences(seed):
    steps, expected, calls, info = batch_run(seed)
    for op in BATCH_OWNERS:
        rows = {h: (shrinks(hist), empty_among(hist)) for h, hist in calls[op].items()}
        assert any(a and b for a, b in rows.values()), (op, rows)
    # the collapse at EVERY grain, each on one workspace: a smaller run after a larger, an empty one between two that are not
    for grain in (F.TAXID, F.TAXID_GI, F.LONG):
        rows = {h: (shrinks(hist), empty_among(hist)) for (h, g), hist in calls["collapse"].items() if g == grain}
        assert any(a and b for a, b in rows.values()), (grain, rows)
    # ... and a workspace whose grain changes between two runs, in both directions
    changing = {h for (h, _) in calls["collapse"] if len({g for (x, g) in calls["collapse"] if x == h}) == 3}
    assert changing == {"runA"}
    # the kinds of operation and of batch the list must hold
    ops = {s["op"] for s in steps}
    assert ops >= {"upload", "run", "run_host", "run_host_parts", "set_verify_mode", "set_assignments", "set_assignment_grain", "set_match_flags",
                   "set_taxa_report", "taxa_report", "take_reads", "copy_reads", "take_unique", "merge_runs", "add_run", "refuse"}
    assert {s["params"] for s in steps if "params" in s} == {"default", "stress", "dense"}
    assert {s["keep"] for s in steps if s["op"] == "take_reads"} == {0, 1}
    assert any(s["op"] == "taxa_report" and s["reset"] for s in steps)
    uploads = [s["reads"] for s in steps if s["op"] == "upload"]
    assert any(len(b) == 0 for b in uploads) and any(b"" in b for b in uploads) and any(0 < len(r) < 18 for b in uploads for r in b)
    assert any(320 < len(r) < 32768 for b in uploads for r in b)
    assert {s["why"] for s in steps if s["op"] == "refuse"} >= {"the grain while the assignments are on", "download_assignments while off",
                                                                "add_run after a host run", "a read of 32 768 bases"}
    # a take from a host batch, and a run on a batch that a take left empty
    assert any(s["op"] == "take_reads" and s["src"] == "runA" for s in steps)
    assert any(s["op"] == "take_reads" and e["result"][0] == 0 for s, e in zip(steps, expected))


WHY_EMPTY = {"reads that hit nothing", "no read survived the take", "a batch of zero reads"}


@pytest.mark.parametrize("seed", LC.BATCH_SEEDS)
def test_no_batch_step_is_trivial(seed):
    """every run, host batch and merge finds something, and not what the step before it on that workspace found -- but for the
    steps the generator wrote to find nothing, which say so and why"""
    steps, expected, _, info = batch_run(seed)
    model = LM.BatchModel(LC.WORKSPACES, None, info["fold_grain"], oracles=LC.oracles())   # (a second model: the hits behind MATCH_ONLY and ASSIGN_ONLY)
    last, empty = {}, 0
    for k, s in enumerate(steps):
        model.apply(s)
        if s["op"] not in ("run", "run_host", "run_host_parts", "merge_runs"):
            continue
        hits = model.w[s["w"]].last["hits"]
        if "why_empty" in s:
            assert s["why_empty"] in WHY_EMPTY and len(hits) == 0, (k, LC.brief(s))
            empty += 1
        else:
            assert len(hits) > 0, (k, LC.brief(s))
            before = last.get(s["w"])
            assert before is None or not LM.same_hits(before, hits), (k, LC.brief(s))
        last[s["w"]] = hits
    assert empty >= 8


def test_the_batch_model_equals_the_restatements_it_wraps():
    import assign_ref as A
    import chain_ref as CR
    import chunk_merge_ref as CM
    import taxa_report_ref as R
    orc = LC.oracles()
    rng = LC.random.Random(5)
    reads = LC.gen_batch(300, rng, 77)
    m = LM.BatchModel({"a": "A", "b": "B", "c": "A", "d": "A"}, None, F.TAXID, oracles=orc)
    for s in ({"op": "set_assignments", "w": "a", "mode": 1}, {"op": "set_match_flags", "w": "a", "mode": 1}, {"op": "set_taxa_report", "w": "a", "on": 1},
              {"op": "upload", "w": "a", "reads": reads}, {"op": "run", "w": "a", "params": "default"}):
        e = m.apply(s)
    hits, _ = orc.hits("A", [LM.letters(r) for r in reads], "default")
    seen = e["seen"]["a"]
    assert len(hits) > 100 and LM.same_hits(seen.hits, hits)
    assert seen.assign == LM.as_array(F.TAXID, A.collapse(hits)).tobytes()
    assert seen.report == R.classify_hits(hits) and seen.flags[1] == len(set(hits["read"].tolist()))
    # the unmatched reads handed on, binned against the other database: the hits carry the caller's numbers
    e = m.apply({"op": "take_reads", "w": "b", "src": "a", "keep": 0})
    codes, off, rmap = CR.compact(CR.normalise(np.frombuffer(b"".join(reads), dtype=np.uint8)), LM.batch_arrays(reads)[1], ~seen.flags[0])
    assert e["result"] == (len(rmap), len(codes)) and e["seen"]["b"].resident == (codes.tobytes(), off.tolist(), rmap.tolist())
    e = m.apply({"op": "run", "w": "b", "params": "default"})
    kept = [LM.letters(reads[j]) for j in rmap.tolist()]
    want, _ = orc.hits("B", kept, "default")
    assert len(want) > 50 and e["seen"]["b"].hits["read"].tolist() == rmap[want["read"].astype(np.int64)].tolist()
    # a merge of two runs over the same reads
    for s in ({"op": "copy_reads", "w": "c", "src": "b"}, {"op": "run", "w": "c", "params": "stress"}, {"op": "merge_runs", "w": "d", "srcs": ["b", "c"]}):
        e = m.apply(s)
    assert LM.same_hits(e["seen"]["d"].hits, CM.merge_hits([m.w["b"].last["hits"], m.w["c"].last["hits"]]))
    # the second run replaces the first; the report adds up until it is reset
    e = m.apply({"op": "run", "w": "a", "params": "stress"})
    assert e["seen"]["a"].report[1] == seen.report[1] + len(set(orc.hits("A", [LM.letters(r) for r in reads], "stress")[0]["read"].tolist()))
    assert m.apply({"op": "taxa_report", "w": "a", "reset": 1})["result"] == e["seen"]["a"].report
    assert m.apply({"op": "taxa_report", "w": "a", "reset": 0})["result"] == ({}, 0)
    # what the header refuses
    assert m.refusal({"op": "set_assignment_grain", "w": "a", "grain": 2}) == LM.E_ARG
    assert m.refusal({"op": "download_assignments", "w": "b", "wide": False}) == LM.E_ARG
    assert m.refusal({"op": "set_match_flags", "w": "a", "mode": 2}) == LM.E_ARG
    assert m.refusal({"op": "take_reads", "w": "a", "src": "d", "keep": 0}) == LM.E_ARG
    assert m.refusal({"op": "run_host", "w": "a", "reads": [b"A" * 32768], "params": "default"}) == LM.E_LIMIT
    assert m.refusal({"op": "run_host", "w": "a", "reads": [b"A" * 32767], "params": "default"}) is None
