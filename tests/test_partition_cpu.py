"""mtsv-partition (the standalone tool) against the Python restatement of partition_ref.py, and the argument rules of
mtsv-binner --matched / --unmatched that are decided before any device call.  No GPU needed."""
import gzip
import os
import subprocess

import pytest

import partition_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PARTITION = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-partition")
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")

# header variants, cycled over the reads: (separator, what follows it in the file)
HEADER_VARIANTS = [
    (b"", b""),                                     # no description
    (b" ", b"some description"),                    # space
    (b"\t", b"after a tab"),                        # tab
    (b" ", b"note:with:colons x=1"),                # a description containing ':'
    (b" ", b"trailing blanks \t "),                 # trailing whitespace is dropped
    (b" ", b""),                                    # a separator and nothing behind it: no description
    (b"\t", b"two  words\tand a tab"),              # inner whitespace is kept
]
QUAL_ALPHABET = b"ABCDEFGHIJ0123456789#$%&"


def golden_reads():
    return [l.rstrip("\n").encode("latin-1") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]


def golden_records(fastq):
    """(records as the restatement sees them, the header lines as they stand in the file)"""
    recs, headers = [], []
    for i, seq in enumerate(golden_reads()):
        sep, tail = HEADER_VARIANTS[i % len(HEADER_VARIANTS)]
        rid = b"r%d" % i
        headers.append(rid + sep + tail)
        qual = bytes(QUAL_ALPHABET[(i + k) % len(QUAL_ALPHABET)] for k in range(len(seq))) if fastq else None
        recs.append((rid, tail.rstrip(P.WHITESPACE), seq, qual))
    return recs, headers


def write_input(path, recs, headers, fastq, gz, wrap=60):
    chunks = []
    for (rid, desc, seq, qual), h in zip(recs, headers):
        if fastq:
            chunks.append(b"@" + h + b"\n" + seq + b"\n+\n" + qual + b"\n")
        else:                                        # wrapped FASTA lines
            chunks.append(b">" + h + b"\n" + b"".join(seq[k:k + wrap] + b"\n" for k in range(0, len(seq), wrap)))
    data = b"".join(chunks)
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(data)


def run_partition(*args):
    return subprocess.run([PARTITION, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_restatement_splits_headers_as_the_binner_reads_ids():
    assert P.split_header(b"r1") == (b"r1", b"")
    assert P.split_header(b"r1 a b ") == (b"r1", b"a b")
    assert P.split_header(b"r1\ta b") == (b"r1", b"a b")
    assert P.split_header(b"r1  x") == (b"r1", b" x")            # one separator only
    assert P.split_header(b"r1 \t ") == (b"r1", b"")
    recs, headers = golden_records(True)
    for (rid, desc, _, _), h in zip(recs, headers):
        assert P.split_header(h) == (rid, desc)
    assert P.record_bytes((b"a", b"", b"ACgt", None), False) == b">a\nACgt\n"
    assert P.record_bytes((b"a", b"d e", b"ACgt", b"IIII"), True) == b"@a d e\nACgt\n+\nIIII\n"


@pytest.mark.parametrize("results_name", ["e2e_default.results", "e2e_default_long.results"])
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gzip"])
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_partition_of_the_golden_reads_equals_the_restatement(tmp_path, fastq, gz, results_name):
    recs, headers = golden_records(fastq)
    reads = [r[2] for r in recs]
    assert any(len(r) > 60 for r in reads) and any(any(c in b"acgtn" for c in r) for r in reads)   # wrapped lines, lowercase
    results = os.path.join(GOLD, results_name)
    ids = P.ids_from_results([open(results, "rb").read()])
    # the fixture cannot degenerate: the golden results name some of the reads and not all of them
    all_ids = {r[0] for r in recs}
    assert ids and ids < all_ids and len(all_ids) == len(recs)
    want_m, want_u = P.partition_by_ids(recs, ids, fastq)
    assert want_m and want_u
    inp = tmp_path / ("reads" + (".fastq" if fastq else ".fasta") + (".gz" if gz else ""))
    write_input(inp, recs, headers, fastq, gz)
    m, u = tmp_path / "matched", tmp_path / "unmatched"
    m.write_bytes(b"stale")                          # the outputs are truncated
    r = run_partition("--results", results, "--fastq" if fastq else "--fasta", inp, "--matched", m, "--unmatched", u)
    assert r.returncode == 0, r.stdout + r.stderr
    got_m, got_u = m.read_bytes(), u.read_bytes()
    assert got_m == want_m and got_u == want_u
    # matched and unmatched are disjoint and together are the input's records in order
    per_rec = [P.record_bytes(rec, fastq) for rec in recs]
    flags = [rec[0] in ids for rec in recs]
    assert b"".join(b for b, f in zip(per_rec, flags) if f) == got_m
    assert b"".join(b for b, f in zip(per_rec, flags) if not f) == got_u
    assert len(got_m) + len(got_u) == sum(map(len, per_rec)) and 0 < sum(flags) < len(flags)


def small_fastq(tmp_path, ids):
    recs = [(i, b"", b"ACGTACGTAC", b"IIIIIIIIII") for i in ids]
    p = tmp_path / "small.fastq"
    write_input(p, recs, [r[0] for r in recs], True, False)
    return recs, p


def test_results_parsing(tmp_path):
    recs, fq = small_fastq(tmp_path, [b"a", b"b:c", b"d", b"e", b"b", b"a"])
    r1, r2 = tmp_path / "r1.txt", tmp_path / "r2.txt"
    r1.write_bytes(b"\n  \t \nb:c:5=1,7=2\r\n\n")            # blank lines; an ID containing ':' (the last ':' splits); CRLF
    r2.write_bytes(b"a:1-2-3=0\nzz:9=9")                     # a second file; no newline at its end; an ID no read carries
    ids = P.ids_from_results([r1.read_bytes(), r2.read_bytes()])
    assert ids == {b"b:c", b"a", b"zz"}
    want_m, want_u = P.partition_by_ids(recs, ids, True)
    m, u = tmp_path / "m", tmp_path / "u"
    # both spellings of several results files
    for argv in (["--results", r1, r2], ["--results", r1, "--results", r2], [f"--results={r1}", "--results", r2]):
        r = run_partition(*argv, "--fastq", fq, "--matched", m, "--unmatched", u)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (m.read_bytes(), u.read_bytes()) == (want_m, want_u)
    # the two records with ID "a" share a fate; "b" alone is not "b:c"
    assert want_m.count(b"@a\n") == 2 and b"@b\n" in want_u and b"@b:c\n" in want_m


@pytest.mark.parametrize("bad", [b"a:1=1\nno colon here\n", b":1=2\n", b"a:1=1\n \n:\n"], ids=["no_colon", "empty_id", "lone_colon"])
def test_invalid_results_lines_exit_2(tmp_path, bad):
    _, fq = small_fastq(tmp_path, [b"a"])
    res = tmp_path / "bad.txt"
    res.write_bytes(bad)
    with pytest.raises(P.InvalidHeader):
        P.ids_from_results([bad])
    r = run_partition("--results", res, "--fastq", fq, "--matched", tmp_path / "m", "--unmatched", tmp_path / "u")
    assert r.returncode == 2
    assert "Unable to parse results: InvalidHeader(" in r.stdout + r.stderr
    assert not (tmp_path / "m").exists()


def test_exit_codes(tmp_path):
    _, fq = small_fastq(tmp_path, [b"a"])
    res = tmp_path / "res.txt"
    res.write_bytes(b"a:1=0\n")
    m, u = tmp_path / "m", tmp_path / "u"
    ok = ["--results", res, "--fastq", fq, "--matched", m, "--unmatched", u]
    assert run_partition(*ok).returncode == 0
    # missing required flags, conflicting inputs, unknown flags: usage errors
    for drop in ("--results", "--fastq", "--matched", "--unmatched"):
        k = ok.index(drop)
        assert run_partition(*(ok[:k] + ok[k + 2:])).returncode == 1, drop
    assert run_partition(*ok, "--fasta", fq).returncode == 1
    assert run_partition(*ok, "--threads", "4").returncode == 1
    assert run_partition("--results").returncode == 1
    assert run_partition("--help").returncode == 0 and run_partition("-V").returncode == 0
    # a results file that cannot be read: exit 2; a reads file that cannot be read, or is broken: exit 3
    assert run_partition("--results", tmp_path / "none.txt", "--fastq", fq, "--matched", m, "--unmatched", u).returncode == 2
    r = run_partition("--results", res, "--fastq", tmp_path / "none.fastq", "--matched", m, "--unmatched", u)
    assert r.returncode == 3 and "Error partitioning reads: " in r.stdout + r.stderr
    broken = tmp_path / "broken.fastq"
    broken.write_bytes(b"@a\nACGT\n+\nII\n")
    assert run_partition("--results", res, "--fastq", broken, "--matched", m, "--unmatched", u).returncode == 3
    # an output that cannot be created: exit 3
    assert run_partition("--results", res, "--fastq", fq, "--matched", tmp_path / "no_dir" / "m", "--unmatched", u).returncode == 3


def test_binner_argument_rules_are_decided_before_any_device_call(tmp_path):
    """every one of these runs names an index file that does not exist: a run that got as far as loading it would exit 2"""
    def binner(*args):
        return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)
    m, u, res = tmp_path / "m", tmp_path / "u", tmp_path / "res"
    base = ["--fastq", tmp_path / "x.fastq", "-i", tmp_path / "no.idx"]
    # --report needs the gathered hits: not without --results
    r = binner(*base, "--matched", m, "--report", tmp_path / "rep.tsv")
    assert r.returncode == 1 and "--report" in r.stderr and "--results" in r.stderr
    # a list of index chunks
    r = binner("--fastq", tmp_path / "x.fastq", "-i", f"{tmp_path}/a.idx,{tmp_path}/b.idx", "-m", res, "--matched", m, "--unmatched", u)
    assert r.returncode == 1 and "index chunks" in r.stderr
    # a results file that the run would resume
    res.write_bytes(b"r0:1=0\n")
    r = binner(*base, "-m", res, "--unmatched", u)
    assert r.returncode == 1 and "resume" in r.stderr
    assert not m.exists() and not u.exists()
    assert res.read_bytes() == b"r0:1=0\n"
    # nothing changes without the new flags: no results path is still exit 3, with --report too
    assert binner(*base).returncode == 3
    assert binner(*base, "--report", tmp_path / "rep.tsv").returncode == 3
    # with them a missing --results is no error of its own: the run gets as far as its input
    assert binner(*base, "--matched", m).returncode == 2
    assert "--matched" in binner("--help").stdout
