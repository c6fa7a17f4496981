"""CPU tests of the pileup (mtsv_pileup, mtsv_format_variants, mtsv-binner --variants): the restatement pile_ref against its
own invariants on every crafted hit, the cases of test_pile.py against what they are meant to reach, the formatter, the ABI,
and the command line's usage errors, which are decided before a device is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mtsv_tools_amd as M
import pile_cases as PL
import pile_ref as PR
import place_cases as PC
import place_ref as R
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


@pytest.fixture(scope="module")
def crafted():
    entries = PC.database()
    reads, hits = PC.crafted(entries)
    hits = PL.with_more_hits(reads, hits)
    return entries, reads, hits, PL.Placer(entries)(reads, hits)


def test_every_crafted_hit_walks_as_the_definition_says(crafted):
    entries, reads, hits, placed = crafted
    assert len(hits) >= 250
    for h, (start, end, ops) in zip(hits, placed):
        r, t, g, o, e, strand = h
        L_ref = PC.BIN_LEN
        slots = [[0] * 8 for _ in range(L_ref + 1)]
        touched, consumed = PR.walk(slots, reads[r], strand, start, ops)
        assert touched == list(range(start, end))                                  # contiguous from ref_start, ref_end - ref_start of them
        assert consumed == len(reads[r]) == sum(n for n, op in ops if op != R.OP_D)  # X + '=' + I bases
        assert sum(PR.depth(n) for n in slots) == end - start
        assert slots[L_ref][:7] == [0] * 7 and end <= L_ref                        # slot L takes only n[7]; nothing beyond it
        assert sum(n[7] for n in slots) == sum(1 for _, op in ops if op == R.OP_I)


def test_slack_and_taxa_select_hits(crafted):
    entries, reads, hits, placed = crafted
    by_read = {}
    for h in hits:
        by_read.setdefault(h[0], []).append(h[4])
    assert sum(len(v) == 3 for v in by_read.values()) == 12
    n = {s: sum(PR.counted(hits, s)) for s in (0, 1, 2, PR.SLACK_ALL)}
    assert n[0] == len(hits) - 24 and n[1] == n[0] + 12 and n[2] == n[PR.SLACK_ALL] == len(hits)
    table = PR.new_table(entries, taxa={2})
    assert sorted(table) == [(2, 20), (2, 21)]
    piled, skipped = PR.add_run(table, reads, hits, placed, PR.SLACK_ALL)
    assert piled + skipped == len(hits) and skipped == sum(h[1] != 2 for h in hits) > 0


def test_the_deep_pile_counts_what_was_planted():
    entries = PC.database()
    reads, hits, planted = PL.deep_pile(entries)
    assert len(hits) == 1000
    table = PR.new_table(entries)
    assert PR.add_run(table, reads, hits, PL.Placer(entries)(reads, hits), 0) == (1000, 0)
    slots = table[PL.DEEP_KEY]
    snp, dele, ins = slots[planted["snp"]], slots[planted["del"]], slots[planted["ins"]]
    assert PR.depth(snp) == 1000 and snp[1 + planted["snp_base"]] == 300 and snp[0] == 700
    assert dele[6] == 100 and PR.depth(dele) == 1000 and ins[7] == 50
    seq = PL.seq_of(entries)
    assert (PL.DEEP_KEY[0], PL.DEEP_KEY[1], planted["snp"]) in {r[:3] for r in PR.sites(table, seq, 0, 0, 300000)}
    assert (PL.DEEP_KEY[0], PL.DEEP_KEY[1], planted["snp"]) not in {r[:3] for r in PR.sites(table, seq, 0, 0, 300001)}
    assert (PL.DEEP_KEY[0], PL.DEEP_KEY[1], planted["snp"]) not in {r[:3] for r in PR.sites(table, seq, 0, 301, 0)}
    assert PR.sites(table, seq, 1001, 0, 0) == []
    assert len(PR.sites(table, seq)) == PL.DEEP_LEN                               # every touched slot


def test_the_slot_l_read_touches_slot_l():
    entries = PC.database()
    read, hit = PL.slot_l_read(entries)
    (start, end, ops), = PL.Placer(entries)([read], [hit])
    table = PR.new_table(entries)
    PR.walk(table[PL.SLOT_L_KEY], read, 0, start, ops)
    assert end == PC.BIN_LEN and ops[-1] == (1, R.OP_I)
    assert table[PL.SLOT_L_KEY][PC.BIN_LEN] == [0, 0, 0, 0, 0, 0, 0, 1]
    rows = PR.sites(table, PL.seq_of(entries))
    assert rows[-1][2] == PC.BIN_LEN and rows[-1][3] == PR.REF_NONE and PR.text(rows).splitlines()[-1].split("\t")[3] == "."


# ---- the formatter ----

def site_rows(rows):
    a = np.zeros(len(rows), dtype=M.PILE_SITE_DTYPE)
    for k, (t, g, pos, ref, n) in enumerate(rows):
        a[k] = (t, g, pos, ref, n)
    return a


FORMAT_ROWS = [
    (1, 10, 0, 0, [5, 0, 1, 0, 0, 0, 0, 0]),
    (1, 10, 7, 1, [0, 2, 0, 0, 0, 0, 0, 0]),
    (2, 20, 4199, 2, [1, 0, 0, 0, 3, 0, 0, 0]),
    (2, 20, 4200, 0xff, [0, 0, 0, 0, 0, 0, 0, 9]),                                 # slot L
    (3, 30, 17, 3, [0, 0, 0, 0, 0, 1, 1, 0]),
    (3, 30, 18, 4, [7, 0, 0, 0, 0, 0, 0, 2]),                                      # a reference N
    (4000000000, 4294967295, 4294967294, 0, [4294967295, 4000000000, 0, 0, 0, 0, 4294967295, 1234567890]),   # counts of 10 digits
]


def test_format_variants_is_the_restatements_text():
    want = PR.text(FORMAT_ROWS)
    assert M.format_variants(site_rows(FORMAT_ROWS)) == want
    assert M.format_variants(site_rows([])) == PR.HEADER == "taxid\tgi\tpos\tref\tdepth\tmatch\tA\tC\tG\tT\tN\tdel\tins\n"
    assert "\t4200\t.\t0\t0\t0\t0\t0\t0\t0\t0\t9\n" in want and "\t12589934590\t4294967295\t4000000000\t" in want
    assert [l.split("\t")[3] for l in want.splitlines()[1:]] == list("ACG.TNA")
    for k, row in enumerate(FORMAT_ROWS):
        assert M.format_variants(site_rows([row])) == PR.HEADER + PR.line(*row)


def test_the_abi_of_the_pileup():
    assert M.PILE_SITE_DTYPE.itemsize == 48 and M.PILE_SITE_DTYPE.fields["n"][1] == 16 and C.sizeof(M.PileupInfo) == 48
    L = M.lib()
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    names = ("mtsv_pileup_create", "mtsv_pileup_free", "mtsv_pileup_reset", "mtsv_pileup_add_run", "mtsv_pileup_info", "mtsv_pileup_download",
             "mtsv_pileup_sites", "mtsv_format_variants")
    for name in names:
        assert name in src and name in _lib.EXPORTS and hasattr(L, name)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mtsv_pileup_create(0, None, 0, None) == _lib.E_ARG
    assert L.mtsv_pileup_create(0, None, 3, C.byref(out)) == _lib.E_ARG
    assert L.mtsv_pileup_add_run(None, None, None, 0, 0, None, None, None) == _lib.E_ARG
    assert L.mtsv_pileup_sites(None, 0, 0, 0, C.byref(out), C.byref(n), None) == _lib.E_ARG
    assert L.mtsv_format_variants(None, 1, C.byref(out), C.byref(n)) == _lib.E_ARG


# ---- the command line ----

def test_binner_usage_errors_of_variants(tmp_path):
    base = ["--fastq", "x.fq", "-i", "a.idx,b.idx", "-m", str(tmp_path / "r")]
    var = ["--variants", str(tmp_path / "var.tsv")]
    fold = ["--fold-on-gpu"]
    cases = [
        (var, "'--variants <TSV>' requires '--fold-on-gpu'"),
        (var + ["--merge-on-gpu"], "'--variants <TSV>' requires '--fold-on-gpu'"),
        (var + fold + ["--dedup"], "'--variants <TSV>' cannot be used with '--dedup': only the representatives"),
        (["--variants", str(tmp_path / "r")] + fold, "'--variants <TSV>' and '-m/--results <RESULTS>' name the same file"),
        (var + fold + ["--alignments", str(tmp_path / "var.tsv")], "'--variants <TSV>' and '--alignments <FILE>' name the same file"),
        (fold + ["--variants"], "requires a value"),
        (fold + ["--variant-taxa", "1,2"], "The argument '--variant-taxa <T1,T2,..>' requires '--variants <TSV>'"),
        (fold + ["--variant-slack", "1"], "The argument '--variant-slack <N|all>' requires '--variants <TSV>'"),
        (fold + ["--min-depth", "2"], "The argument '--min-depth <N>' requires '--variants <TSV>'"),
        (fold + ["--min-alt-reads", "2"], "The argument '--min-alt-reads <N>' requires '--variants <TSV>'"),
        (fold + ["--min-alt-frac", "0.5"], "The argument '--min-alt-frac <F>' requires '--variants <TSV>'"),
        (var + fold + ["--min-alt-frac", "1.5"], "Invalid value for '--min-alt-frac <F>': a fraction between 0 and 1 is expected"),
        (var + fold + ["--min-alt-frac", "x"], "Invalid value for '--min-alt-frac <F>'"),
        (var + fold + ["--min-depth", "-1"], "Invalid value for '--min-depth <N>'"),
        (var + fold + ["--variant-slack", "some"], "Invalid value for '--variant-slack <N>'"),
        (var + fold + ["--variant-taxa", "1,,2"], "Invalid value for '--variant-taxa <T1,T2,..>': a comma-separated list of TaxIDs is expected"),
        (var + fold + ["--variant-taxa", "1,x"], "Invalid value for '--variant-taxa <T1,T2,..>'"),
    ]
    for args, message in cases:
        r = subprocess.run([BINNER, *base, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert not (tmp_path / "var.tsv").exists() and not (tmp_path / "r").exists()
    r = subprocess.run([BINNER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--variants TSV [--variant-taxa T1,T2,..] [--variant-slack N|all] [--min-depth N] [--min-alt-reads N]" in r.stdout
    assert "33 bytes" in r.stdout
