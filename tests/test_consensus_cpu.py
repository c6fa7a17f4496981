"""CPU tests of the consensus (mtsv_pileup_consensus, mtsv_format_consensus_stats, mtsv_pileup_add_counts, mtsv-binner
--consensus): the restatement cons_ref on the strain's reads -- the condition the GPU round trip relies on --, the rows'
invariants, the edge tables against what they are meant to reach, the formatter, the ABI, and the command line's usage errors,
which are decided before a device is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cons_cases as CC
import cons_ref as CR
import mtsv_tools_amd as M
import pile_cases as PL
import pile_ref as PR
import place_cases as PC
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


@pytest.fixture(scope="module")
def strained():
    entries = PC.database()
    st = CC.strain(entries)
    table = PR.new_table(entries)
    piled, skipped = PR.add_run(table, st["reads"], st["hits"], PL.Placer(entries)(st["reads"], st["hits"]), 0)
    assert (piled, skipped) == (len(st["hits"]), 0)
    return entries, st, table


def test_the_strains_reads_spell_the_strain(strained):
    entries, st, table = strained
    seq = PL.seq_of(entries)
    key, lo, hi = st["key"], st["lo"], st["hi"]
    assert all(60 <= len(r) <= 100 for r in st["reads"]) and {h[5] for h in st["hits"]} == {0, 1}
    assert min(PR.depth(n) for n in table[key][lo:hi]) >= CC.STRAIN_DEPTH
    assert len(st["snps"]) == 5 and all(abs(a - b) > 1 for a in st["snps"] for b in st["snps"] if a != b)
    for fill in (CR.FILL_N, CR.FILL_REF):
        chars, row = CR.call_reference(table[key], seq[key], CC.STRAIN_DEPTH, 500000, fill)
        ref = seq[key].decode()
        outside = (lambda s: "N" * len(s)) if fill == CR.FILL_N else (lambda s: s.lower())
        assert chars == outside(ref[:lo]) + st["expected"] + outside(ref[hi:])
        assert len(st["expected"]) == hi - lo - 1                                  # the deletion is applied, the insertion absent
        assert (row["n_sub"], row["n_del"], row["ins_sites"], row["n_ambig"]) == (5, 1, 1, 0)
        assert row["covered"] == hi - lo and row["n_low"] == len(ref) - (hi - lo) and row["n_ref"] == hi - lo - 6
    slots = table[key]
    assert 2 * slots[st["ins"]][7] > PR.depth(slots[st["ins"]]) and slots[st["dele"]][6] == max(slots[st["dele"]][:7])
    text, rows = CR.consensus(table, seq, CC.STRAIN_DEPTH)
    assert [r[:2] for r in rows] == [key] and text.startswith(">%d-%d\n" % (key[1], key[0]))
    assert text.split("\n", 1)[1].replace("\n", "").strip("N") == st["expected"]
    assert all(len(l) == 60 for l in text.splitlines()[1:-1]) and text.endswith("\n") and "\n\n" not in text


def test_the_rows_invariants_on_the_crafted_hits():
    entries = PC.database()
    reads, hits = PC.crafted(entries)
    hits = PL.with_more_hits(reads, hits)
    table = PR.new_table(entries)
    PR.add_run(table, reads, hits, PL.Placer(entries)(reads, hits), PR.SLACK_ALL)
    seq = PL.seq_of(entries)
    for params in ((1, 500000, 0, 0, 60), (0, 0, 0, 1, 0), (2, 1000000, 100000, 1, 7), (1, 500000, 1000000, 0, 1)):
        text, rows = CR.consensus(table, seq, *params)                             # (asserts both sums of every reference)
        assert [r[:2] for r in rows] == sorted(r[:2] for r in rows) and text.count(">") == len(rows)
        for r in rows:
            row = dict(zip(CR.FIELDS, r))
            assert row["length"] == PC.BIN_LEN == row["covered"] + row["n_low"]
            assert row["covered"] == row["n_ref"] + row["n_sub"] + row["n_del"] + row["n_ambig"] >= 1
    # (2, 21) takes no crafted hit: covered 0, never emitted
    assert [r[:2] for r in CR.consensus(table, seq, 1, 500000, 0)[1]] == [(1, 10), (2, 20), (3, 30)] and CR.consensus(table, seq, 1, 500000, 1000000) == ("", [])


def test_the_edge_slots_reach_what_they_are_meant_to():
    kind = lambda p, md=2, ppm=500000: CR.classify(CC.EDGE_SLOTS[p], md, ppm)
    assert kind(0) == (CR.REF, 0) and kind(1) == (CR.SUB, 1) and kind(2) == (CR.SUB, 4)
    assert kind(3) == (CR.REF, 0) and kind(3, 2, 500001)[0] == CR.AMBIG
    assert kind(4)[0] == CR.AMBIG and kind(5) == (CR.REF, 0) and kind(6) == (CR.AMBIG, 5)
    assert kind(7, 3)[0] == CR.REF and kind(7, 4)[0] == CR.LOW and kind(8, 2)[0] == CR.REF and kind(8, 3)[0] == CR.LOW
    assert kind(13) == (CR.DEL, 6) and kind(14)[0] == CR.LOW and kind(15) == (CR.SUB, 2)
    seq = b"ACGT" * 16
    slots = CC.edge_table(len(seq))
    zero, one = (CR.call_reference(slots, seq, md, 500000, 0) for md in (0, 1))
    assert zero == one and one[1]["covered"] == 15                                 # min_depth 0 behaves as 1
    row = CR.call_reference(slots, seq, 2, 500000, 0)[1]
    # INS SITES at min_depth 2: positions 11, 12 and 14, and slot L; not 10, where 2 * ins == depth
    assert row["ins_sites"] == 4 and CR.call_reference(CC.edge_table(len(seq), 0), seq, 2, 500000, 0)[1]["ins_sites"] == 3
    assert CR.call_reference(slots, seq, 4, 500000, 0)[1]["ins_sites"] == 1        # only position 14: 5 reads
    tables = CC.random_tables(CC.small_database())
    assert all(max(max(n) for n in t) <= CC.ADD_HITS and t[-1][:7] == [0] * 7 for t in tables.values())
    chars, row = CR.call_reference(tables[(3, 30)], b"ACGTACGTA", 1, 500000, 0)
    assert chars == "" and row["n_del"] == 9 and CR.wrap("", 60) == "" and CR.wrap("", 0) == ""
    assert CR.wrap("ACGT", 4) == "ACGT\n" and CR.wrap("ACGTA", 4) == "ACGT\nA\n" and CR.wrap("ACG", 4) == "ACG\n" and CR.wrap("ACGTACGT", 4) == "ACGT\nACGT\n"
    assert CR.wrap("ACGT", 0) == "ACGT\n" and CR.wrap("ACG", 1) == "A\nC\nG\n"


# ---- the formatter ----

def cons_rows(rows):
    a = np.zeros(len(rows), dtype=M.CONS_REF_DTYPE)
    for k, r in enumerate(rows):
        a[k] = r
    return a


FORMAT_ROWS = [
    # tax_id, gi, length, covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites, sum_depth
    (1, 10, 4200, 600, 594, 5, 1, 3600, 0, 1, 4711),
    (1, 11, 3, 1, 0, 0, 0, 2, 1, 0, 2),                                            # nothing called: identity 0.00
    (2, 20, 0, 0, 0, 0, 0, 0, 0, 1, 0),                                            # no base at all: every ratio 0.00
    (7, 1, 9, 9, 0, 0, 9, 0, 0, 0, 36),                                            # deleted at every position: cons_len 0
    (7, 4294967295, 4294967294, 4294967294, 4000000000, 294967294, 0, 0, 0, 4294967295, 18446744073709551615 - 36),   # (the TaxID sums stay within 64 bits)
    (4000000000, 5, 100, 50, 25, 12, 13, 50, 0, 0, 333),
]


def test_format_consensus_stats_is_the_restatements_text():
    assert M.CONS_REF_DTYPE.itemsize == 48 and M.CONS_REF_DTYPE.fields["sum_depth"][1] == 40
    want = CR.stats_text(FORMAT_ROWS)
    assert M.format_consensus_stats(cons_rows(FORMAT_ROWS)) == want
    assert M.format_consensus_stats(cons_rows([])) == CR.HEADER
    assert CR.HEADER == "taxid\tgi\tlength\tcovered\tbreadth_pct\tmean_depth\tcons_len\tref\tsub\tdel\tlow\tambiguous\tins_sites\tidentity_pct\n"
    lines = want.splitlines()
    assert len(lines) == 1 + len(FORMAT_ROWS) + 4                                  # a rollup per TaxID
    assert lines[1] == "1\t10\t4200\t600\t14.29\t1.12\t4199\t594\t5\t1\t3600\t0\t1\t99.00"
    assert lines[2].endswith("\t0.00") and lines[3] == "1\t*\t4203\t601\t14.30\t1.12\t4202\t594\t5\t1\t3602\t1\t1\t99.00"
    assert lines[4] == "2\t20\t0\t0\t0.00\t0.00\t0\t0\t0\t0\t0\t0\t1\t0.00" and lines[5].startswith("2\t*\t0\t")
    assert lines[6].split("\t")[6] == "0" and lines[6].endswith("\t0.00")
    assert lines[8].startswith("7\t*\t4294967303\t4294967303\t")
    for row in FORMAT_ROWS:
        assert M.format_consensus_stats(cons_rows([row])) == CR.HEADER + CR.stats_line(*row) + CR.stats_line(row[0], "*", *row[2:])


def test_the_abi_of_the_consensus():
    L = M.lib()
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    for name in ("mtsv_pileup_consensus", "mtsv_format_consensus_stats", "mtsv_pileup_add_counts"):
        assert name in src and name in _lib.EXPORTS and hasattr(L, name)
    assert "} mtsv_cons_ref; /* 48 bytes */" in src and "INSERTIONS CANNOT BE SPELLED" in src
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    assert L.mtsv_pileup_consensus.argtypes == [vp, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
    assert L.mtsv_format_consensus_stats.argtypes == [vp, u64, C.POINTER(vp), C.POINTER(u64)]
    assert L.mtsv_pileup_add_counts.argtypes == [vp, u32, u32, u32, u64, vp, u64]
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mtsv_pileup_consensus(None, 1, 500000, 0, 0, 60, C.byref(out), C.byref(n), None, None, None) == _lib.E_ARG
    assert L.mtsv_pileup_add_counts(None, 1, 1, 0, 0, None, 0) == _lib.E_ARG
    assert L.mtsv_format_consensus_stats(None, 1, C.byref(out), C.byref(n)) == _lib.E_ARG
    assert L.mtsv_format_consensus_stats(None, 0, None, C.byref(n)) == _lib.E_ARG


# ---- the command line ----

def test_binner_usage_errors_of_consensus(tmp_path):
    base = ["--fastq", "x.fq", "-i", "a.idx,b.idx", "-m", str(tmp_path / "r")]
    cons = ["--consensus", str(tmp_path / "cons.fa")]
    stats = ["--consensus-stats", str(tmp_path / "cons.tsv")]
    fold = ["--fold-on-gpu"]
    cases = [
        (cons, "'--consensus <FASTA>' requires '--fold-on-gpu'"),
        (cons + ["--merge-on-gpu"], "'--consensus <FASTA>' requires '--fold-on-gpu'"),
        (cons + fold + ["--dedup"], "'--consensus <FASTA>' cannot be used with '--dedup': only the representatives"),
        (["--consensus", str(tmp_path / "r")] + fold, "'--consensus <FASTA>' and '-m/--results <RESULTS>' name the same file"),
        (cons + fold + ["--alignments", str(tmp_path / "cons.fa")], "'--consensus <FASTA>' and '--alignments <FILE>' name the same file"),
        (cons + fold + ["--variants", str(tmp_path / "cons.fa")], "'--consensus <FASTA>' and '--variants <TSV>' name the same file"),
        (cons + fold + ["--consensus-stats", str(tmp_path / "cons.fa")], "'--consensus-stats <TSV>' and '--consensus <FASTA>' name the same file"),
        (cons + fold + ["--consensus-stats", str(tmp_path / "r")], "'--consensus-stats <TSV>' and '-m/--results <RESULTS>' name the same file"),
        (cons + stats + fold + ["--variants", str(tmp_path / "cons.tsv")], "'--consensus-stats <TSV>' and '--variants <TSV>' name the same file"),
        (fold + ["--consensus"], "requires a value"),
        (fold + stats, "The argument '--consensus-stats <TSV>' requires '--consensus <FASTA>'"),
        (fold + ["--consensus-min-depth", "2"], "The argument '--consensus-min-depth <N>' requires '--consensus <FASTA>'"),
        (fold + ["--consensus-min-frac", "0.5"], "The argument '--consensus-min-frac <F>' requires '--consensus <FASTA>'"),
        (fold + ["--consensus-min-breadth", "0.5"], "The argument '--consensus-min-breadth <F>' requires '--consensus <FASTA>'"),
        (fold + ["--consensus-fill", "ref"], "The argument '--consensus-fill <n|ref>' requires '--consensus <FASTA>'"),
        (fold + ["--consensus-width", "70"], "The argument '--consensus-width <N>' requires '--consensus <FASTA>'"),
        (fold + ["--variant-taxa", "1,2"], "The argument '--variant-taxa <T1,T2,..>' requires '--variants <TSV>'"),
        (cons + fold + ["--consensus-min-frac", "1.5"], "Invalid value for '--consensus-min-frac <F>': a fraction between 0 and 1 is expected"),
        (cons + fold + ["--consensus-min-breadth", "x"], "Invalid value for '--consensus-min-breadth <F>'"),
        (cons + fold + ["--consensus-min-depth", "-1"], "Invalid value for '--consensus-min-depth <N>'"),
        (cons + fold + ["--consensus-width", "wide"], "Invalid value for '--consensus-width <N>'"),
        (cons + fold + ["--consensus-fill", "x"], "Invalid value for '--consensus-fill <n|ref>': 'n' or 'ref' is expected"),
        (cons + fold + ["--variant-taxa", "1,,2"], "Invalid value for '--variant-taxa <T1,T2,..>': a comma-separated list of TaxIDs is expected"),
        (cons + fold + ["--variant-slack", "some"], "Invalid value for '--variant-slack <N>'"),
        (cons + fold + ["--min-depth", "2"], "The argument '--min-depth <N>' requires '--variants <TSV>'"),
    ]
    for args, message in cases:
        r = subprocess.run([BINNER, *base, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and message in r.stderr, (args, r.stderr)
        assert not (tmp_path / "cons.fa").exists() and not (tmp_path / "cons.tsv").exists() and not (tmp_path / "r").exists()
    r = subprocess.run([BINNER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--consensus FASTA [--consensus-stats TSV] [--consensus-min-depth N] [--consensus-min-frac F]" in r.stdout
    assert "cannot be spelled" in r.stdout
