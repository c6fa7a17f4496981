"""-m gpu tests of the alignments of hits (k_place.hip, mtsv_batch_place_hits, mtsv-binner --alignments).

Crafted hits go in through mtsv_batch_place_hits(hits != NULL), so the kernel is tested without binning; real runs place
the hits where they lie on the device.  Expected values never come from the device: they are place_ref's -- the whole matrix,
column by column, and a traceback.  Every comparison is exact: start, end, the number of ops and the ops themselves.
MTSV_PLACE_RING is read by a workspace's first call, so every case makes its own workspace under each setting."""
import os
import random
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import place_cases as PC
import place_ref as R
from mtsv_tools_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
RINGS = {"ring_min": "1", "ring_4096": "4096"}                # (forced up to what the call needs; 4096 never wraps but for the far matches)
STRESS = dict(max_hits=5, tune_max_hits=2, max_candidates=3, max_assignments=1, min_seed=0.5)
KEYS = ("read", "tax_id", "gi", "edit", "strand")


def fields(a):
    """a structured array field by field (the padding of a copy holds anything)"""
    return [a[name].tolist() for name in a.dtype.names]


def same(pl, ops, hits, want):
    """placements and ops against the hits they describe and place_ref's (start, end, ops) of each"""
    assert len(pl) == len(hits) == len(want)
    for k in KEYS:
        assert (pl[k] == hits[k]).all(), k
    for k, (p, w) in enumerate(zip(pl, want)):
        lo, n = int(p["ops_off"]), int(p["n_ops"])
        got = (int(p["ref_start"]), int(p["ref_end"]), ops[lo:lo + n].tolist())
        assert got == (w[0], w[1], R.encode(w[2])), (k, hits[k], got, w)
        assert n <= 2 * int(hits["edit"][k]) + 1
    spans = sorted((int(p["ops_off"]), int(p["ops_off"]) + int(p["n_ops"])) for p in pl)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= len(ops))


def workspace(ix, reads, monkeypatch, ring="ring_min", **kw):
    monkeypatch.setenv("MTSV_PLACE_RING", RINGS[ring])
    bases, off = helpers.reads_to_batch(reads)
    b = M.Batch(ix, 0, max(len(reads), 1), max(len(bases), 1), **kw)
    b.upload(bases, off)
    return b


@pytest.fixture(scope="module")
def crafted():
    entries = PC.database()
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    reads, hits = PC.crafted(entries)
    return ix, entries, reads, hits, PC.expected(entries, reads, hits)


# ---- 1. crafted hits ----

@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("longest", [64, 65, 128, 129, 161, 224, 256])        # k_place<2> .. k_place<8>
def test_crafted_hits_by_template_width(crafted, longest, ring, monkeypatch):
    ix, entries, reads, hits, want = crafted
    keep = [k for k, h in enumerate(hits) if len(reads[h[0]]) <= longest]
    sub_reads = [reads[hits[k][0]] for k in keep]
    assert max(len(r) for r in sub_reads) == longest
    sub_hits = PC.hits_array([(j,) + hits[k][1:] for j, k in enumerate(keep)], M.HIT_DTYPE)
    b = workspace(ix, sub_reads, monkeypatch, ring)
    pl, ops, ms = b.place_hits(sub_hits)
    same(pl, ops, sub_hits, [want[k] for k in keep])
    assert ms > 0
    b.close()


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_batch_sizes(crafted, n, monkeypatch):
    ix, entries, reads, hits, want = crafted
    order = [(7 * k) % len(hits) for k in range(n)]                            # any order, hits repeated
    h = PC.hits_array([hits[k] for k in order], M.HIT_DTYPE)
    b = workspace(ix, reads, monkeypatch)
    pl, ops, ms = b.place_hits(h)
    same(pl, ops, h, [want[k] for k in order])
    assert (ms > 0) == (n > 0) and (n > 0 or len(ops) == 0)
    pl2, ops2, _ = b.place_hits(h)                                             # the workspace's arrays are reused
    assert fields(pl2) == fields(pl) and ops2.tobytes() == ops.tobytes()
    b.close()


# ---- 2. refusals ----

def refused(b, hits, code, *words):
    with pytest.raises(M.MtsvError) as e:
        b.place_hits(hits)
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_workspace_as_it_was(crafted, monkeypatch):
    ix, entries, reads, hits, want = crafted
    text_of = {(t, g): s for t, g, s in entries}
    good = PC.hits_array(hits, M.HIT_DTYPE)
    b = workspace(ix, reads, monkeypatch)

    def one_bad(k, **field):
        h = good.copy()
        for name, v in field.items():
            h[name][k] = v
        return h

    k = max(range(len(hits)), key=lambda i: hits[i][4])                        # the heaviest script
    r, t, g, o, e, strand = hits[k]
    m = R.min_edit(R.strand_codes(reads[r], strand), R.codes(text_of[(t, g)][o:]))  # over everything behind the offset
    assert 1 <= m <= e
    first = f"the first is hit {k} (read {r}, tax_id {t}, gi {g}, strand {strand}"
    refused(b, one_bad(k, edit=m - 1), _lib.E_ARG, "1 of %d hits are unplaceable" % len(hits), first, f"edit {m - 1}) at offset {o}")
    same(*b.place_hits(one_bad(k, edit=m))[:2], one_bad(k, edit=m), want[:k] + [R.place_hit(reads[r], strand, text_of[(t, g)], o, m)] + want[k + 1:])
    refused(b, one_bad(5, gi=999), _lib.E_ARG, "1 name a (tax_id, gi) the index does not hold, 0 lie", "the first is hit 5 ", "gi 999")
    refused(b, one_bad(9, offset=PC.BIN_LEN), _lib.E_ARG, "0 name a (tax_id, gi)", "1 lie at or beyond the end of their bin", "the first is hit 9 ")
    refused(b, one_bad(3, read=len(reads)), _lib.E_ARG, "1 name a read that is not resident", "the first is hit 3 (read %d," % len(reads))
    refused(b, one_bad(3, read=1 << 40), _lib.E_ARG, "1 name a read that is not resident")
    refused(b, one_bad(70, strand=2), _lib.E_ARG, "1 carry a strand above 1", "the first is hit 70 ")
    h = one_bad(2, gi=1)
    h["offset"][100] = 1 << 33
    h["strand"][1] = 9
    refused(b, h, _lib.E_ARG, "1 name a (tax_id, gi)", "1 lie at or beyond", "1 carry a strand", "the first is hit 1 ")
    refused(b, None, _lib.E_ARG, "no completed run")                           # hits == NULL needs a run
    same(*b.place_hits(good)[:2], good, want)                                  # ... and a valid call is a fresh workspace's
    fresh = workspace(ix, reads, monkeypatch)
    (pl_f, ops_f, _), (pl_b, ops_b, _) = fresh.place_hits(good), b.place_hits(good)
    assert fields(pl_f) == fields(pl_b) and ops_f.tobytes() == ops_b.tobytes()
    fresh.close()
    b.close()


def test_refusals_of_the_index_and_the_batch(crafted, monkeypatch):
    ix, entries, reads, hits, want = crafted
    one = PC.hits_array(hits[:1], M.HIT_DTYPE)
    twice = M.MGIndex.build([(1, 10, entries[0][2]), (2, 20, entries[1][2]), (1, 10, entries[2][2])], threads=2)
    twice.to_device(0)
    b = workspace(twice, reads, monkeypatch)
    refused(b, one, _lib.E_ARG, "the index holds (tax_id 1, gi 10) in two bins")
    refused(b, one[:0], _lib.E_ARG, "in two bins")
    b.close()
    twice.close()
    long_reads = reads[:3] + [helpers.rnd_seq(random.Random(1), 257)]
    b = workspace(ix, long_reads, monkeypatch)
    refused(b, one, _lib.E_LIMIT, "a read of 257 bases", "up to 256")
    b.close()
    b = M.Batch(ix, 0, 16, 4096)
    refused(b, one, _lib.E_ARG, "holds no resident batch")
    bases, off = helpers.reads_to_batch(reads[:4])
    b.run_host(bases, off)
    refused(b, None, _lib.E_ARG, "host batch")
    b.close()


# ---- 3. real runs ----

@pytest.fixture(scope="module")
def tricky():
    entries, gene, unit = helpers.tricky_db(seed=7)
    ix = M.MGIndex.build(entries, threads=4)
    ix.to_device(0)
    reads = helpers.tricky_reads(entries, gene, unit, seed=11, n_each=24)
    return ix, entries, reads, {}


def expected_of(hits, entries, reads, cache):
    text_of = {(t, g): s for t, g, s in entries}
    out = []
    for h in hits:
        key = tuple(int(h[k]) for k in KEYS) + (int(h["offset"]),)
        if key not in cache:
            r, t, g, e, strand, o = key
            cache[key] = R.place_hit(reads[r], strand, text_of[(t, g)], o, e)
        out.append(cache[key])
    assert all(w is not None for w in out)
    return out


def state_of(b, mode, n_reads):
    """what a placement must not change: the hits, the statistics, the assignments and a fold of the run"""
    out = [fields(b.download()), sorted(b.stats().items())]
    if mode != M.ASSIGN_OFF:
        out.append(fields(b.download_assignments()[0]))
        fold = M.Fold(0, M.GRAIN_TAXID, n_reads=n_reads)
        fold.add_run(b)
        out.append(fields(fold.download()))
        fold.close()
    return out


@pytest.mark.parametrize("pname", ["default", "stress"])
@pytest.mark.parametrize("kw", [{}, {"max_hits_ws": 64}], ids=["one_pass", "several_passes"])
def test_the_hits_of_a_run_where_they_lie(tricky, pname, kw, monkeypatch):
    ix, entries, reads, cache = tricky
    mp = M.default_params(**(STRESS if pname == "stress" else {}))
    hits_by_mode = {}
    for mode in (M.ASSIGN_OFF, M.ASSIGN_ONLY):
        b = workspace(ix, reads, monkeypatch, **kw)
        b.set_assignments(mode)
        b.run(mp)
        before = state_of(b, mode, len(reads))
        pl, ops, ms = b.place_hits()
        assert state_of(b, mode, len(reads)) == before
        hits = b.download()
        if mode == M.ASSIGN_ONLY:                              # the hits stay on the device: the other mode's are the same run's
            assert len(hits) == 0
            hits = hits_by_mode[M.ASSIGN_OFF]
        hits_by_mode[mode] = hits
        assert len(hits) > 10 and ms > 0
        same(pl, ops, hits, expected_of(hits, entries, reads, cache))
        b.close()


def test_a_mapped_workspace(tricky, monkeypatch):
    ix, entries, reads, cache = tricky
    rng = random.Random(3)
    some = [e for e in entries if len(e[2]) > 400][:3]
    filt = M.MGIndex.build([(1, 1, helpers.rnd_seq(rng, 3000))] + some, threads=2)
    filt.to_device(0)
    src = workspace(filt, reads, monkeypatch)
    src.set_match_flags(M.MATCH_ONLY)
    src.run()
    dst = M.Batch(ix, 0, len(reads), sum(len(r) for r in reads))
    n_kept, _, _ = dst.take_reads(src, M.KEEP_UNMATCHED)
    assert 0 < n_kept < len(reads)
    dst.run()
    hits = dst.download()
    assert len(hits) > 20 and int(hits["read"].max()) >= n_kept            # the caller's numbers, not the resident ones
    pl, ops, _ = dst.place_hits()
    want = expected_of(hits, entries, reads, cache)
    same(pl, ops, hits, want)
    pl2, ops2, _ = dst.place_hits(hits[::-1].copy())                        # given hits carry the caller's numbers too
    same(pl2, ops2, hits[::-1], want[::-1])
    gone = sorted(set(range(len(reads))) - set(dst.read_map().tolist()))[0]
    bad = hits[:1].copy()
    bad["read"] = gone
    refused(dst, bad, _lib.E_ARG, "1 name a read that is not resident", f"(read {gone},")
    for w in (src, dst, filt):
        w.close()


# ---- 4. mtsv-binner --fold-on-gpu --alignments ----

@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("place_e2e")
    chunks = [PC.database(seed=5, first_tax=1), PC.database(seed=6, first_tax=11)]
    reads, ids = PC.paired_reads(chunks)
    fq = d / "reads.fastq"
    with open(fq, "wb") as f:
        for r, i in zip(reads, ids):
            f.write(b"@" + i.encode() + b" some description\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    bases, off = helpers.reads_to_batch(reads)
    paths, lines = [], []
    for c, entries in enumerate(chunks):
        ix = M.MGIndex.build(entries, threads=4)
        paths.append(str(d / f"chunk{c}.idx"))
        ix.write(paths[-1])
        ix.to_device(0)
        b = M.Batch(ix, 0, len(reads), len(bases), lanes=1)
        b.upload(bases, off)
        b.run()
        hits = b.download()
        b.close()
        ix.close()
        for h, (start, end, ops) in zip(hits, expected_of(hits, entries, reads, {})):
            lines.append(R.line(ids[int(h["read"])], int(h["tax_id"]), int(h["gi"]), int(h["strand"]), start, end, int(h["edit"]), ops))
    assert len(lines) >= len(reads) // 2 and any("\t-\t" in x for x in lines) and any("X" in x or "I" in x or "D" in x for x in lines)
    return d, ",".join(paths), fq, sorted(lines)


@pytest.mark.parametrize("flags", [["--output-format", "long"], ["--interleaved"], ["--output-format", "long", "--batch-reads", "16", "--fold-reads", "40"]],
                         ids=["long", "interleaved", "many_super_batches"])
def test_binner_alignments_are_the_restatements_lines(flags, e2e, tmp_path):
    d, index, fq, want = e2e
    out = {}
    for name, extra in (("with", ["--alignments", tmp_path / "aln.tsv"]), ("without", [])):
        res, rep, cov = (tmp_path / f"{name}.{x}" for x in ("res", "report", "cov"))
        r = subprocess.run([BINNER, *map(str, ["--fastq", fq, "-i", index, "-m", res, "--report", rep, "--coverage", cov, "--fold-on-gpu", *flags, *extra])],
                           capture_output=True, text=True, timeout=600, env={**os.environ, "MTSV_CLI_TIMING": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = (res.read_bytes(), rep.read_bytes(), cov.read_bytes())
        assert ("[cli alignments timing] alignments %d," % len(want) in r.stderr) == bool(extra)
    assert out["with"] == out["without"] and len(out["with"][0]) > 0
    got = sorted((tmp_path / "aln.tsv").read_text().splitlines(keepends=True))
    assert got == want
