"""-m gpu tests of result text parsed on the device (k_parse.hip, mtsv_fold_add_text, mtsv-collapse --on-gpu).

Expected records never come from the device or from the code under test: they are parse_ref.records (pinned against the
host mtsv-collapse by test_parse_text_cpu.py) of the same lines, or the host tool's own output.  Every comparison is exact."""
import random
import re

import numpy as np
import pytest

import fold_ref as F
import mtsv_tools_amd as M
import parse_cases as PC
import parse_ref as P
import text_cases as T
from mtsv_tools_amd import _lib
from test_fold import as_array, check_fold, records_of

pytestmark = pytest.mark.gpu

GRAINS = T.GRAINS


def raw(fold):
    return (fold.download() if fold.grain == F.TAXID else fold.download_gi()).tobytes()


def add(fold, lines):
    return fold.add_text(*P.arrays(lines))


def n_tokens(lines):
    return sum(len(h.split(",")) for _, h in lines if h)


def refused(fold, lines, code, line, n_reads=None):
    """the call fails with `code`, names `line`, and leaves count and download as they were"""
    before = (fold.count(), raw(fold))
    with pytest.raises(M.MtsvError) as e:
        add(fold, lines)
    assert e.value.code == code, e.value
    assert f"line {line}:" in str(e.value), e.value
    assert (fold.count(), raw(fold)) == before


def loaded_fold(grain, n_reads=50):
    fold = M.Fold(0, grain, n_reads=n_reads)
    have = [T.rec(grain, 1, 5, 6, 7, 8), T.rec(grain, 4, 5, 6, 7, 2), T.rec(grain, 4, 9, 1, 1, 0)]
    fold.add_records(as_array(grain, have))
    return fold, have


# ---- 1. tile edges ----

@pytest.mark.parametrize("tile", ["64", None], ids=["tile64", "default_tile"])
@pytest.mark.parametrize("gname", list(GRAINS))
def test_tokens_at_every_offset_of_a_tile(gname, tile, monkeypatch, capfd):
    grain = GRAINS[gname]
    if tile:
        monkeypatch.setenv("MTSV_PARSE_TILE", tile)
    else:
        monkeypatch.delenv("MTSV_PARSE_TILE", raising=False)
    monkeypatch.setenv("MTSV_TRACE", "1")
    lines = PC.edge_lines()                                                    # (its coverage of a tile: test_parse_text_cpu.py)
    n_reads = lines[-1][0] + 1
    want = P.records(grain, lines, n_reads)
    fold = M.Fold(0, grain, n_reads=n_reads)
    monkeypatch.setenv("MTSV_PARSE_TILE", "128")                               # (read when the fold was created, not later)
    tok, rec, ms = add(fold, lines)
    assert (tok, rec) == (n_tokens(lines), len(want)) and ms >= 0.0
    check_fold(fold, want, n_reads)
    tok2, rec2, _ = add(fold, lines)                                           # the same text again changes nothing
    assert (tok2, rec2) == (tok, rec)
    check_fold(fold, want, n_reads)
    fold.close()
    tiles = set(re.findall(r"\[parse\] \d+ bytes in \d+ lines -> \d+ tokens -> \d+ records in \d+ tiles of (\d+) bytes", capfd.readouterr().err))
    assert tiles == {tile or "4096"}


def test_taxid_fold_takes_all_three_shapes(monkeypatch):
    monkeypatch.setenv("MTSV_PARSE_TILE", "64")
    lines = []
    for r, h in PC.edge_lines(seed=12, n_lines=200):
        toks = h.split(",") if h else []
        shaped = []
        for k, t in enumerate(toks):
            left, edit = t.split("=")
            parts = left.split("-")
            shaped.append("-".join(parts[:1 + (k + r) % 3]) + "=" + edit)
        lines.append((r, ",".join(shaped)))
    n_reads = lines[-1][0] + 1
    want = P.records(F.TAXID, lines, n_reads)
    assert {t.count("-") for _, h in lines if h for t in h.split(",")} == {0, 1, 2}
    fold = M.Fold(0, F.TAXID, n_reads=n_reads)
    assert add(fold, lines)[:2] == (n_tokens(lines), len(want))
    check_fold(fold, want, n_reads)
    fold.close()


# ---- 2. numbers ----

@pytest.mark.parametrize("gname", list(GRAINS))
def test_smallest_and_largest_numbers(gname):
    grain = GRAINS[gname]
    vals = (0, 9, 10, 4294967295)
    lines = [(k, f"{v}-{v}-{v}={v}") for k, v in enumerate(vals)]
    if grain == F.TAXID:
        lines += [(4, "0=0,9=9,10=10,4294967295=4294967295")]
    fold = M.Fold(0, grain, n_reads=5)
    add(fold, lines)
    want = [T.rec(grain, k, v, v, v, v) for k, v in enumerate(vals)] + ([(4, v, v) for v in vals] if grain == F.TAXID else [])
    assert P.records(grain, lines, 5) == want
    check_fold(fold, want, 5)
    fold.close()


BAD_NUMBERS = ["4294967296", "9999999999", "12345678901"]
BAD_TOKENS = ([f"{s}=1" for s in BAD_NUMBERS] + [f"1={s}" for s in BAD_NUMBERS] + [f"1-{s}-1=1" for s in BAD_NUMBERS] + [f"1-1-{s}=1" for s in BAD_NUMBERS] +
              ["=5", "5=", "1--3=4", "5==3", "1-2-3-4=5", "1a=2", "1-b-3=2", "1 =2", " 1=2", "1=2 ", "1=2\r", "\r1=2"])


@pytest.mark.parametrize("bad", BAD_TOKENS, ids=[repr(b) for b in BAD_TOKENS])
def test_token_outside_the_grammar_is_refused(bad):
    fold, have = loaded_fold(F.TAXID)
    with pytest.raises(P.Format):
        P.records(F.TAXID, [(0, bad)], 50)
    for lines, line in (([(0, "1=1"), (2, ""), (3, f"2=2,{bad}"), (7, "3=3"), (9, bad)], 2),
                        ([(0, bad)], 0),
                        ([(0, "1=1,2=2"), (6, f"{bad},7=7")], 1)):
        refused(fold, lines, _lib.E_FORMAT, line)
    check_fold(fold, have, 50)
    fold.close()


# ---- 3. shapes ----

def test_no_lines_one_line_and_empty_lines():
    for grain in GRAINS.values():
        fold, have = loaded_fold(grain)
        assert fold.add_text(b"", np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))[:2] == (0, 0)
        assert add(fold, [(3, ""), (3, ""), (2, "")])[:2] == (0, 0)           # empty lines only: their reads are not looked at
        check_fold(fold, have, 50)
        one = [(7, "3-2-1=0")]
        assert add(fold, one)[:2] == (1, 1)
        want = F.fold(grain, have, P.records(grain, one, 50))
        check_fold(fold, want, 50)
        lines = [(0, ""), (1, ""), (2, "5-6-7=1"), (9, ""), (9, ""), (11, "1-1-1=1,1-1-2=0"), (30, ""), (49, "2-2-2=2"), (49, ""), (3, "")]
        add(fold, lines)
        want = F.fold(grain, want, P.records(grain, lines, 50))
        check_fold(fold, want, 50)
        fold.close()


def test_order_and_range_of_the_reads_and_keys():
    for grain in GRAINS.values():
        fold, have = loaded_fold(grain)
        ok = "1-1-1=1"
        for lines, line in (([(3, ok), (3, ok)], 1),                               # equal
                            ([(3, ok), (5, ""), (2, ok)], 2),                      # descending, over an empty line
                            ([(0, ok), (50, ok)], 1),                              # at n_reads
                            ([(4000000000, ok)], 0),
                            ([(1, ok), (2, "2-1-1=1,1-9-9=1"), (3, "2-1-1=1,1-9-9=1")], 1)):   # keys descend
            with pytest.raises(P.Arg) as e:
                P.records(grain, lines, 50)
            assert e.value.line == line
            refused(fold, lines, _lib.E_ARG, line)
        if grain != F.TAXID:
            refused(fold, [(1, "2-1-9=1,2-1-1=1" if grain == F.LONG else "2-5-1=1,2-1-1=1")], _lib.E_ARG, 0)
            for short in ("1=2", "1-2=3"):                                         # a wide grain needs GI and offset
                refused(fold, [(0, ok), (1, f"{ok},{short}")], _lib.E_FORMAT, 1)
        blob, off, reads = P.arrays([(1, ok), (2, ok)])
        for bad_off in (np.array([0, 9, 7], dtype=np.uint64), np.array([1, 7, 14], dtype=np.uint64)):
            before = raw(fold)
            with pytest.raises(M.MtsvError) as e:
                fold.add_text(blob, bad_off, reads)
            assert e.value.code == _lib.E_ARG and raw(fold) == before
        check_fold(fold, have, 50)
        fold.close()


# ---- 4. reduction ----

def deep_line():
    """5000 long tokens of one TaxID: GI runs of 1 to 40 tokens, offsets ascending inside a run with exact repeats, edits that
    tie; runs that straddle tokens 256, 1024, 2048 and 4096 of the call"""
    rng = random.Random(70)
    toks, gi = [], 0
    while len(toks) < 5000:
        gi += rng.randrange(1, 3)
        n = (1, 2, 3, 5, 7, 40)[gi % 6]
        offs = sorted(rng.randrange(0, 60) * 1000 for _ in range(n))
        toks += [(gi, o, rng.randrange(0, 4)) for o in offs]
    toks = toks[:5000]
    return toks


def test_a_line_of_5000_tokens_of_one_taxid():
    toks = deep_line()
    first = [(2, "1-1-1=3,7-0-0=9")]                                                # 2 tokens before the deep line
    for edge in (256, 1024, 2048, 4096):                                           # token `edge` of the call continues a (TaxID, GI) run
        assert toks[edge - 2 - 1][0] == toks[edge - 2][0]
    pairs = list(zip(toks, toks[1:]))
    assert any(a[:2] == b[:2] and a[2] != b[2] for a, b in pairs)                   # one long key twice, two edits
    assert any(a[0] == b[0] and a[1] != b[1] and a[2] == b[2] == min(t[2] for t in toks if t[0] == a[0]) for a, b in pairs)  # tied edits, two offsets
    lines = first + [(3, ",".join(f"7-{g}-{o}={e}" for g, o, e in toks)), (5, "7-1-1=1")]
    assert len(lines[1][1]) > 8 * 4096
    for grain in GRAINS.values():
        want = P.records(grain, lines, 6)
        n3 = sum(r[0] == 3 for r in want)
        assert n3 == {F.TAXID: 1, F.TAXID_GI: len({t[0] for t in toks}), F.LONG: len({t[:2] for t in toks})}[grain]
        fold = M.Fold(0, grain, n_reads=6)
        assert add(fold, lines)[:2] == (5003, len(want))
        check_fold(fold, want, 6)
        fold.close()


# ---- 5. round trip ----

@pytest.mark.parametrize("gname", list(GRAINS))
def test_text_written_on_the_device_parses_back_to_its_records(gname):
    grain = GRAINS[gname]
    cases = T.cases(grain)
    for name in ("ladder", "later_fields", "size_1", "size_65", "one_read_of_six_tiles", "single_record_reads", "many_long_ids"):
        if name not in cases:
            continue
        c = cases[name]
        n_reads = len(c.ids)
        src = M.Fold(0, grain, n_reads=n_reads)
        src.add_records(as_array(grain, c.records))
        text = src.format_text(c.table)[0]
        src.close()
        assert text == T.expected(grain, c)
        reads = sorted({r[0] for r in c.records})
        rows = text.decode().splitlines()
        assert len(rows) == len(reads)
        lines = [(read, row.rsplit(":", 1)[1]) for read, row in zip(reads, rows)]
        dst = M.Fold(0, grain, n_reads=n_reads)
        assert add(dst, lines)[:2] == (len(c.records), len(c.records)), name
        assert records_of(dst) == c.records, name
        dst.close()


# ---- 6. fold equivalence ----

@pytest.mark.parametrize("gname", list(GRAINS))
def test_texts_of_three_chunks_fold_like_their_records(gname):
    grain = GRAINS[gname]
    chunks = [PC.edge_lines(seed=s, n_lines=150) for s in (21, 22, 23)]
    n_reads = max(c[-1][0] for c in chunks) + 1
    lists = [P.records(grain, c, n_reads) for c in chunks]
    assert len({r[0] for r in lists[0]} & {r[0] for r in lists[1]} & {r[0] for r in lists[2]}) > 5
    for order in ((0, 1, 2), (2, 1, 0)):
        a, b = M.Fold(0, grain, n_reads=n_reads), M.Fold(0, grain, n_reads=n_reads)
        for k in order:
            add(a, chunks[k])
            b.add_records(as_array(grain, lists[k]))
            assert raw(a) == raw(b)
        check_fold(a, F.fold_all(grain, lists), n_reads)
        a.close()
        b.close()


# ---- 7. the command line ----

def both(tmp_path, texts, mode, env=None, fallback=False):
    """mtsv-collapse without and with --on-gpu: the same output and report, byte for byte; returns the device run's stderr"""
    h, h_out, h_rep = PC.run_tool(tmp_path, texts, "--mode", mode, tag="host")
    assert h.returncode == 0, h.stderr
    g, g_out, g_rep = PC.run_tool(tmp_path, texts, "--mode", mode, "--on-gpu", "-v", env=dict(env or {}, MTSV_COLLAPSE_TIMING="1"), tag="gpu")
    assert g.returncode == 0, g.stderr
    assert g_out == h_out and g_rep == h_rep and len(h_out) > 0 and len(h_rep) > 0
    assert ("the host path takes the input" in g.stderr) == fallback
    assert ("[collapse timing]" in g.stderr) == (not fallback)
    return g.stderr


@pytest.mark.parametrize("mode", ["taxid", "taxid-gi"])
def test_cli_reference_vectors(mode, tmp_path):
    texts, want = PC.REFERENCE[mode]
    both(tmp_path, texts, mode)
    assert (tmp_path / "gpu.txt").read_text() == want
    if mode == "taxid":
        both(tmp_path, PC.REPORT_INPUT, mode)


@pytest.mark.parametrize("case", ["default/taxid", "long/taxid", "long/taxid-gi/pieces"])
def test_cli_golden_results_cut_into_three_files(case, tmp_path):
    name, mode = case.split("/")[:2]
    texts = PC.golden_cut("e2e_default.results" if name == "default" else "e2e_default_long.results")
    pieces = case.endswith("pieces")
    err = both(tmp_path, texts, mode, env={"MTSV_COLLAPSE_PIECE_BYTES": "256"} if pieces else None)
    calls = int(re.search(r"\[collapse timing\] files 3 reads \d+ calls (\d+) ", err).group(1))
    assert calls > 20 if pieces else calls == 3


@pytest.mark.parametrize("case", ["colon/taxid-gi", "layers/taxid", "layers/taxid-gi"])
def test_cli_ids_with_colons_and_ids_on_several_lines(case, tmp_path):
    name, mode = case.split("/")
    err = both(tmp_path, {"colon": PC.COLON_IDS, "layers": PC.LAYERS}[name], mode)
    calls = int(re.search(r" calls (\d+) ", err).group(1))
    assert calls == (4 if name == "layers" else 2)                              # layers: three of the first file, one of the second


@pytest.mark.parametrize("case", ["key_order", "no_offset"])
def test_cli_input_the_device_refuses_goes_to_the_host_path(case, tmp_path):
    err = both(tmp_path, PC.KEY_ORDER if case == "key_order" else PC.NO_OFFSET, "taxid-gi", fallback=True)
    assert err.count("--on-gpu:") == 1


def test_cli_malformed_token_ends_as_on_the_host(tmp_path):
    h, h_out, _ = PC.run_tool(tmp_path, PC.MALFORMED, "--mode", "taxid-gi", tag="host")
    g, g_out, _ = PC.run_tool(tmp_path, PC.MALFORMED, "--mode", "taxid-gi", "--on-gpu", tag="host")     # (the same file names: the same message)
    assert h.returncode == 101 and (g.returncode, g.stderr) == (h.returncode, h.stderr)
    assert "InvalidInteger(x)" in g.stderr
