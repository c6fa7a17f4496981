"""CPU tests for result text parsed on the device: they pin the restatement parse_ref.py -- which the GPU tests of
test_parse_text.py compare the device with -- against the host mtsv-collapse binary, and check what the new flags decide
before a device is opened.  Nothing here runs the code under test on a device."""
import subprocess

import pytest

import fold_ref as F
import parse_cases as PC
import parse_ref as P
import text_cases as T

MODES = {"taxid": F.TAXID, "taxid-gi": F.TAXID_GI}


def restated(mode, texts):
    ids, recs = P.collapse_files(MODES[mode], texts)
    return T.text(MODES[mode], recs, ids), recs


@pytest.mark.parametrize("mode", list(MODES))
def test_reference_vectors(mode, tmp_path):
    texts, want = PC.REFERENCE[mode]
    r, out, _ = PC.run_tool(tmp_path, texts, "--mode", mode)
    assert r.returncode == 0 and out.decode() == want
    assert restated(mode, texts)[0].decode() == want
    assert restated(mode, texts[::-1])[0].decode() == want


@pytest.mark.parametrize("case", ["default/taxid", "long/taxid", "long/taxid-gi", "colon/taxid", "colon/taxid-gi", "layers/taxid", "layers/taxid-gi",
                                  "edges/taxid", "edges/taxid-gi"])
def test_restatement_gives_the_host_tools_output(case, tmp_path):
    name, mode = case.split("/")
    if name in ("default", "long"):
        texts = PC.golden_cut("e2e_default.results" if name == "default" else "e2e_default_long.results")
    elif name == "edges":
        lines = PC.edge_lines()
        texts = ["".join(f"id{r:05d}:{h}\n" for r, h in lines[:300]), "".join(f"id{r:05d}:{h}\n" for r, h in reversed(lines[200:]))]
    else:
        texts = {"colon": PC.COLON_IDS, "layers": PC.LAYERS}[name]
    r, out, rep = PC.run_tool(tmp_path, texts, "--mode", mode)
    assert r.returncode == 0, r.stderr
    want, recs = restated(mode, texts)
    assert out == want and len(out) > 0
    # the report's rows against fold_ref.report of the restated records
    stats, total = F.report(recs)
    rows = [l.split("\t") for l in rep.decode().splitlines()[1:]]
    assert {int(x[0]): [int(x[1]), int(x[3]), int(x[5]), int(x[7])] for x in rows} == {k: list(v) for k, v in stats.items()}
    assert total == len({r[0] for r in recs})


def test_restatement_refuses_what_the_grammar_excludes():
    for tok in ("4294967296", "9999999999", "12345678901", "", "x", " 1", "1\r"):
        for hits in (f"{tok}=1", f"1={tok}", f"1-{tok}-3=4", f"1-2-{tok}=4"):
            with pytest.raises(P.Format) as e:
                P.records(F.TAXID, [(0, "1=1"), (1, hits)], 5)
            assert e.value.line == 1
    for hits in ("5==3", "1-2-3-4=5", "1=2,", ",1=2", "1=2,,3=4", "1", "="):
        with pytest.raises(P.Format):
            P.records(F.TAXID, [(0, hits)], 5)
    for grain in (F.TAXID_GI, F.LONG):
        for hits in ("1=2", "1-2=3"):
            with pytest.raises(P.Format):
                P.records(grain, [(0, hits)], 5)
    assert P.records(F.TAXID, [(2, "0=0,9-1=9,10-1-1=10,4294967295=4294967295")], 3) == [(2, 0, 0), (2, 9, 9), (2, 10, 10), (2, 4294967295, 4294967295)]
    for lines in ([(1, "1=1"), (1, "2=2")], [(2, "1=1"), (1, "2=2")], [(5, "1=1")], [(0, "2=1,1=1")]):
        with pytest.raises(P.Arg):
            P.records(F.TAXID, lines, 5)
    assert P.records(F.TAXID_GI, [(0, "1-5-3=7,1-5-2=4,1-5-9=4")], 1) == [(0, 1, 5, 2, 4)]
    assert P.records(F.LONG, [(0, "1-5-3=7,1-5-3=4,1-5-9=4")], 1) == [(0, 1, 5, 3, 4), (0, 1, 5, 9, 4)]


def test_edge_text_reaches_every_offset_of_a_tile():
    lines = PC.edge_lines()
    starts, ends, commas, slots = PC.edge_coverage(lines, PC.TILE)
    every = set(range(PC.TILE))
    assert starts == every and ends == every and commas == every
    assert 0 in slots and len(slots) > 32                                   # a line that begins on a tile edge
    assert sum(len(h) for _, h in lines) > 3 * 4096
    assert any(h == "" for _, h in lines)
    assert {len(t) for _, h in lines if h for t in h.split(",")} >= set(range(9, 44))


def test_flags_that_are_decided_before_a_device_is_opened(tmp_path):
    p = tmp_path / "in.txt"
    p.write_text("r1:1=5\n")
    out = tmp_path / "o.txt"

    def run(*args):
        return subprocess.run([PC.BIN, *args], capture_output=True, text=True)

    r = run("-o", str(out), "--device", "0", str(p))                          # --device without --on-gpu
    assert r.returncode == 1 and "--on-gpu" in r.stderr and not out.exists()
    r = run("-o", str(out), "--on-gpu", "--device", "zero", str(p))
    assert r.returncode == 1 and "--device" in r.stderr and not out.exists()
    r = run("-o", str(out), "--on-gpu", "--device")
    assert r.returncode == 1 and "requires a value" in r.stderr
    r = run("--on-gpu", str(p))                                               # no output named
    assert r.returncode == 1
    r = run("--help")
    assert r.returncode == 0 and "--on-gpu" in r.stdout
    r = run("-o", str(out), str(p))                                           # and the tool as it always was
    assert r.returncode == 0 and out.read_text() == "r1:1=5\n"
