"""The drop-in command line (mtsv_tools_amd/bin/mtsv-binner): flags, exit codes and -- on a GPU --
byte-identical result lines for FASTA, FASTQ and gzip input, read offset and resume."""
import gzip
import os
import subprocess

import pytest

import mtsv_tools_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
GOLD = os.path.join(ROOT, "tests", "golden")


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)


def test_exit_codes_without_touching_the_gpu(tmp_path):
    assert run("--fasta", "x").returncode == 1                                  # clap: missing --index
    assert run("--fasta", "x", "--fastq", "y", "-i", "z").returncode == 1      # conflicting inputs
    assert run("--fasta", "x", "-i", "y").returncode == 3                      # no results path (mtsv-binner.rs:264)
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "-e", "1.5").returncode == 101   # panic!: edit rate
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--min-seed", "0").returncode == 101
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--seed-size", "abc").returncode == 101
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--output-format", "xml").returncode == 1
    assert run("--fasta", str(tmp_path / "missing.fa"), "-i", "y", "-m", str(tmp_path / "r")).returncode == 2
    assert "2.1.0" in run("--version").stdout
    # the multi-GPU extras are validated before anything is opened
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--devices", "0,x").returncode == 1
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--devices", "").returncode == 1
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--batch-reads", "0").returncode == 1
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--batch-reads", "many").returncode == 1
    assert run("--fasta", "x", "-i", "y", "-m", str(tmp_path / "r"), "--batch-reads", "-5").returncode == 1


def test_a_doubly_wrong_command_line_gets_the_message_of_the_first_violation(tmp_path):
    """Validation order is part of the interface: of two violations the earlier check's message and exit code come out,
    and a run refused there has touched no output file.  Nothing here opens a device, an index or the input."""
    r, m, rep = str(tmp_path / "r"), str(tmp_path / "m.fq"), str(tmp_path / "rep.tsv")
    existing = tmp_path / "existing.results"
    existing.write_bytes(b"r0:1=0\nr1:2=3\n")
    missing = str(tmp_path / "missing.fa")
    table = [
        # (arguments, exit code, what only the winning message says, what the losing message says)
        (["--fasta", "x", "-i", "a,b", "-m", r, "--text-on-gpu", "--merge-on-gpu"], 1,
         "'--text-on-gpu' cannot be used with '--merge-on-gpu'", "requires '--fold-on-gpu'"),
        (["--fasta", "x", "-i", "a,b", "-m", r, "--fold-on-gpu", "--merge-on-gpu", "--filter-index", "f"], 1,
         "'--merge-on-gpu' cannot be used with '--fold-on-gpu'", "--filter-index"),
        (["--fasta", "x", "-i", "a", "-m", r, "--fold-on-gpu", "--filter-index", "f"], 1,
         "'--filter-index <INDEX>' cannot be used with '--fold-on-gpu'", "two or more index chunks"),
        (["--fasta", "x", "-i", "a", "-m", r, "--merge-on-gpu", "--devices", "0,1"], 1,
         "'--merge-on-gpu' needs a list of two or more index chunks", "exactly one '--devices' entry"),
        (["--fasta", "x", "-i", "a", "-m", r, "--fold-on-gpu", "--devices", "0,1"], 1,
         "'--fold-on-gpu' needs a list of two or more index chunks", "exactly one '--devices' entry"),
        (["--fasta", "x", "-i", "a,b", "-m", r, "--merge-on-gpu", "--devices", "0,1", "--parse-only"], 1,
         "'--merge-on-gpu' needs exactly one '--devices' entry", "--parse-only"),
        (["--fasta", "x", "--matched", m, "--parse-only", "--filter-index", "f"], 1,
         "'--parse-only' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'", "--filter-index"),
        (["--fasta", "x", "-i", "a", "--report", rep, "--matched", m, "--output-format", "xml"], 1,
         "'--report <TSV>' requires '-m/--results <RESULTS>'", "--output-format"),
        (["--fasta", "x", "-i", "a,b", "-m", r, "--report", rep, "--matched", m], 1,
         "'--report <TSV>' cannot be used with a list of index chunks", "'--matched <PATH>' / '--unmatched <PATH>' cannot"),
        (["--fasta", "x", "-i", "a,b", "-m", r, "--filter-index", "f", "--matched", m], 1,
         "'--matched <PATH>' / '--unmatched <PATH>' cannot be used with a list of index chunks", "--filter-index"),
        (["--fasta", "x", "-i", "a", "-m", r, "--output-format", "xml", "--edit-rate", "1.5"], 1,       # usage error before panic
         "'xml' isn't a valid value for '--output-format <OUTPUT_FORMAT>'", "panicked"),
        (["--fasta", "x", "-i", "a", "--edit-rate", "1.5"], 101,                                          # panic before "no results path"
         "Edit tolerance proportion must be between 0 and 1", "No results path"),
        (["--fasta", missing, "-i", "a", "-m", str(existing), "--matched", m], 1,                         # refusal before the input is opened
         "would resume it; '--matched' / '--unmatched' need the whole input", "cannot open"),
        (["--fasta", missing, "-i", "a,b", "-m", str(existing), "--fold-on-gpu"], 1,
         "would resume it; '--fold-on-gpu' does not resume", "cannot open"),
        (["--fasta", "x", "-i", "a", "-m", r, "--output-format=xml", "--edit-rate=1.5"], 1,              # --key=value of a value flag
         "'xml' isn't a valid value for '--output-format <OUTPUT_FORMAT>'", "panicked"),
        (["--fasta", "x", "-i", "a", "-m", r, "--batch-reads=0", "--bogus=1"], 1,
         "Invalid value for '--batch-reads <N>'", "--bogus"),
        (["--fasta", "x", "-i", "a", "-m", r, "--bogus=1", "--batch-reads=0"], 1,                         # ... and of an unknown flag
         "Found argument '--bogus=1' which wasn't expected", "--batch-reads"),
    ]
    for args, code, says, does_not_say in table:
        got = run(*args)
        text = got.stdout + got.stderr
        assert got.returncode == code, (args, text)
        assert says in text and does_not_say not in text, (args, text)
    assert existing.read_bytes() == b"r0:1=0\nr1:2=3\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["existing.results"]  # no results, --matched or report file was made


def _golden_inputs(tmp_path):
    reads = [l.rstrip("\n") for l in open(os.path.join(GOLD, "e2e_reads.txt"), encoding="latin-1")]
    fa, fq = tmp_path / "reads.fasta", tmp_path / "reads.fastq"
    with open(fa, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f">r{i} some description\n")
            for k in range(0, len(r), 60):      # multi-line FASTA
                f.write(r[k:k + 60] + "\n")
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i} desc\n{r}\n+\n{'I' * len(r)}\n")
    fqgz = tmp_path / "reads.fastq.gz"
    with open(fq, "rb") as src, gzip.open(fqgz, "wb") as dst:
        dst.write(src.read())
    idx = tmp_path / "db.idx"
    M.MGIndex.build_fasta(os.path.join(GOLD, "e2e_db.fasta"), threads=4).write(str(idx))
    return reads, str(fa), str(fq), str(fqgz), str(idx)


@pytest.mark.gpu
def test_cli_end_to_end_matches_golden_results(tmp_path):
    reads, fa, fq, fqgz, idx = _golden_inputs(tmp_path)
    want = sorted(open(os.path.join(GOLD, "e2e_default.results")).read().splitlines())
    want_long = sorted(open(os.path.join(GOLD, "e2e_default_long.results")).read().splitlines())
    stress = sorted(open(os.path.join(GOLD, "e2e_stress.results")).read().splitlines())
    for flag, path in (("--fasta", fa), ("--fastq", fq), ("--fastq", fqgz)):
        out = tmp_path / "res.txt"
        r = run(flag, path, "-i", idx, "-m", str(out), "--force-overwrite", "--batch-reads", "50")
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(open(out).read().splitlines()) == want
    out = tmp_path / "long.txt"
    assert run("--fasta", fa, "-i", idx, "-m", str(out), "--output-format", "long").returncode == 0
    assert sorted(open(out).read().splitlines()) == want_long
    out = tmp_path / "stress.txt"
    assert run("--fastq", fq, "-i", idx, "-m", str(out), "--max-hits", "5", "--tune-max-hits", "2", "--max-candidates", "3",
               "--max-assignments", "1", "--min-seed", "0.5").returncode == 0
    assert sorted(open(out).read().splitlines()) == stress


@pytest.mark.gpu
def test_cli_read_offset_and_resume(tmp_path):
    reads, fa, fq, fqgz, idx = _golden_inputs(tmp_path)
    want = open(os.path.join(GOLD, "e2e_default.results")).read().splitlines()
    ids = [int(l.split(":")[0][1:]) for l in want]
    out = tmp_path / "off.txt"
    assert run("--fasta", fa, "-i", idx, "-m", str(out), "--read-offset", "100").returncode == 0
    assert sorted(open(out).read().splitlines()) == sorted(l for l, i in zip(want, ids) if i >= 100)
    # resume (mtsv-binner.rs:347-411): an existing results file holding the lines of the first 120 reads
    part = tmp_path / "resume.txt"
    with open(part, "w") as f:
        f.write("".join(l + "\n" for l, i in zip(want, ids) if i < 120))
    last = max(i for i in ids if i < 120)
    assert run("--fastq", fq, "-i", idx, "-m", str(part)).returncode == 0
    got = open(part).read().splitlines()
    assert sorted(got) == sorted([l for l, i in zip(want, ids) if i < 120] + [l for l, i in zip(want, ids) if i > last])
    # a results file without a read id is a resume error (exit 4)
    bad = tmp_path / "bad.txt"
    bad.write_text("no colon here\n")
    assert run("--fasta", fa, "-i", idx, "-m", str(bad)).returncode == 4


@pytest.mark.gpu
def test_chunk_mode_binner_then_collapse_equals_oracle_per_chunk(tmp_path):
    """BASELINE config 5 on one GPU: the database split into index chunks, the same reads binned
    against every chunk, results merged with mtsv-collapse == per-chunk CPU runs merged the same way."""
    import helpers
    from oracle import oracle as O

    entries, gene, unit = helpers.tricky_db(seed=7)
    reads = [r for r in helpers.tricky_reads(entries, gene, unit, seed=21, n_each=25) if 0 < len(r) <= 253]
    fq = tmp_path / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@q{i}\n{r.decode('latin-1')}\n+\n{'I' * len(r)}\n")
    bases, off = helpers.reads_to_batch(reads)
    collapse = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
    gpu_files, cpu_files = [], []
    for c in range(3):
        chunk = entries[c::3]
        idx = tmp_path / f"chunk{c}.idx"
        M.MGIndex.build(chunk, threads=2).write(str(idx))
        out = tmp_path / f"gpu{c}.txt"
        assert run("--fastq", str(fq), "-i", str(idx), "-m", str(out), "--output-format", "long").returncode == 0
        gpu_files.append(str(out))
        hits, _ = O.Index.read(str(idx)).bin_batch(bases, off, threads=4)
        cpu = tmp_path / f"cpu{c}.txt"
        cpu.write_text("".join(O.format_line(f"q{r}", hits[hits["read"] == r], True) for r in range(len(reads))))
        cpu_files.append(str(cpu))
    for mode in ("taxid", "taxid-gi"):
        a, b = tmp_path / f"g_{mode}.txt", tmp_path / f"c_{mode}.txt"
        assert subprocess.run([collapse, "-o", str(a), "--mode", mode, *gpu_files]).returncode == 0
        assert subprocess.run([collapse, "-o", str(b), "--mode", mode, *cpu_files]).returncode == 0
        assert a.read_text() == b.read_text() and len(a.read_text()) > 200


@pytest.mark.gpu
def test_cli_devices_list_gives_the_single_device_output(tmp_path):
    """Mode A of SURVEY 8(e) in the product: --devices 0,0 = two workers with a workspace each on one GPU
    pulling the read batches; lines and their order equal the single-device run (README.md:69-73 workflow)."""
    import helpers
    entries, gene, unit = helpers.tricky_db(seed=7)
    reads = [r for r in helpers.tricky_reads(entries, gene, unit, seed=33, n_each=40, lengths=(150, 100)) if len(r) > 0]
    fq = tmp_path / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@q{i}\n{r.decode('latin-1')}\n+\n{'I' * len(r)}\n")
    idx = tmp_path / "db.idx"
    M.MGIndex.build(entries, threads=2).write(str(idx))
    one, two, three = tmp_path / "one.txt", tmp_path / "two.txt", tmp_path / "three.txt"
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(one), "--batch-reads", "37").returncode == 0
    r = run("--fastq", str(fq), "-i", str(idx), "-m", str(two), "--batch-reads", "37", "--devices", "0,0")
    assert r.returncode == 0, r.stdout + r.stderr
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(three), "--batch-reads", "11", "--devices", "0,0,0", "--output-format", "long").returncode == 0
    assert one.read_text() == two.read_text() and len(one.read_text()) > 1000
    ref_long = tmp_path / "long.txt"
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(ref_long), "--output-format", "long").returncode == 0
    assert ref_long.read_text() == three.read_text()
    # the reference-order verification gives the same file (the command line defaults to edit-first)
    env = dict(os.environ, MTSV_VERIFY="reference")
    ref = tmp_path / "ref.txt"
    assert subprocess.run([BIN, "--fastq", str(fq), "-i", str(idx), "-m", str(ref)], env=env, capture_output=True).returncode == 0
    assert ref.read_text() == one.read_text()
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(ref), "--devices", "0,x").returncode == 1
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(ref), "--batch-reads", "0").returncode == 1
    assert run("--fastq", str(fq), "-i", str(idx), "-m", str(ref), "--batch-reads", "many").returncode == 1


@pytest.mark.gpu
def test_cli_chunk_list_merges_like_collapse(tmp_path):
    """Mode B of SURVEY 8(e) in the product: --index a,b,c (the chunks of one database) writes ONE results file
    whose collapse equals the collapse of the three per-chunk result files (README.md:189, collapse.rs:597-625)."""
    import helpers
    entries, gene, unit = helpers.tricky_db(seed=7)
    reads = [r for r in helpers.tricky_reads(entries, gene, unit, seed=21, n_each=25) if 0 < len(r) <= 253]
    fq = tmp_path / "reads.fastq"
    with open(fq, "w", encoding="latin-1") as f:
        for i, r in enumerate(reads):
            f.write(f"@q{i}\n{r.decode('latin-1')}\n+\n{'I' * len(r)}\n")
    collapse = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
    idxs, per_chunk = [], []
    for c in range(3):
        idx = tmp_path / f"chunk{c}.idx"
        M.MGIndex.build(entries[c::3], threads=2).write(str(idx))
        idxs.append(str(idx))
        out = tmp_path / f"gpu{c}.txt"
        assert run("--fastq", str(fq), "-i", str(idx), "-m", str(out)).returncode == 0
        per_chunk.append(str(out))
    merged = tmp_path / "merged.txt"
    r = run("--fastq", str(fq), "-i", ",".join(idxs), "-m", str(merged), "--devices", "0,0,0", "--batch-reads", "64")
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    assert subprocess.run([collapse, "-o", str(a), *per_chunk]).returncode == 0
    assert subprocess.run([collapse, "-o", str(b), str(merged)]).returncode == 0
    assert a.read_text() == b.read_text() and len(a.read_text()) > 200
    # the merged file already holds one line per read with the smallest edit per TaxId: collapse changes nothing but order
    assert sorted(merged.read_text().splitlines()) == sorted(b.read_text().splitlines())


def test_mtsv_build_cli_writes_the_reference_layout(tmp_path):
    """bin/mtsv-build (host suffix sort here: --device -1): same bytes as the library builder and the
    oracle's MGIndex::new restatement; header grammar and mapping-file handling of src/io.rs"""
    import helpers
    from oracle import oracle as O

    build = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-build")
    entries, _, _ = helpers.tricky_db(seed=4)
    fa = tmp_path / "db.fasta"
    with open(fa, "w") as f:
        for tax, gi, seq in entries:
            f.write(f">{gi}-{tax} desc\n{seq.decode()}\n")
    out, ref = tmp_path / "cli.idx", tmp_path / "orc.idx"
    r = subprocess.run([build, "-f", str(fa), "-i", str(out), "--device", "-1", "--sa-sample", "16", "--sample-interval", "32"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    O.Index.build(entries, 32, 16).write(str(ref))
    assert open(out, "rb").read() == open(ref, "rb").read()
    # mapping file: header, taxid, seqid columns (any of , tab ; | or whitespace), --skip-missing
    fa2 = tmp_path / "db2.fasta"
    with open(fa2, "w") as f:
        for i, (tax, gi, seq) in enumerate(entries):
            f.write(f">seq{i} x\n{seq.decode()}\n")
        f.write(">unmapped\nACGTACGTACGTACGTACGT\n")
    mp = tmp_path / "map.tsv"
    with open(mp, "w") as f:
        f.write("Header\tTaxID\tSeqID\n")
        for i, (tax, gi, seq) in enumerate(entries):
            f.write(f"seq{i}\t{tax}\t{gi}\n")
    out2 = tmp_path / "cli2.idx"
    r = subprocess.run([build, "-f", str(fa2), "-i", str(out2), "--device", "-1", "--sa-sample", "16", "--sample-interval", "32",
                        "--mapping", str(mp)], capture_output=True, text=True)
    assert r.returncode == 1  # missing mapping for a header
    r = subprocess.run([build, "-f", str(fa2), "-i", str(out2), "--device", "-1", "--sa-sample", "16", "--sample-interval", "32",
                        "--mapping", str(mp), "--skip-missing"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out2, "rb").read() == open(ref, "rb").read()
    assert subprocess.run([build, "-f", str(fa), "-i", str(out), "--sa-sample", "x"], capture_output=True).returncode == 101
    assert subprocess.run([build, "-f", str(tmp_path / "nope.fa"), "-i", str(out), "--device", "-1"], capture_output=True).returncode == 101


@pytest.mark.gpu
def test_parallel_ingest_and_formatting_equal_the_serial_pipeline(tmp_path):
    """150 k reads: several ingest blocks (1 MiB), several batches, result formatting split over host
    threads (>= 65536 hits per batch).  Output must be byte-identical, in order, to the single-threaded
    serial pipeline, and as a set of lines to the oracle's formatter over the oracle's hits."""
    import numpy as np
    from oracle import oracle as O

    ix = M.MGIndex.synth(77, 8, 2, 20000, threads=4)
    idx = tmp_path / "p.idx"
    ix.write(str(idx))
    bases, off = M.synth_reads(ix, 3, 150000, 100)
    lens = np.diff(off)
    fq = tmp_path / "p.fastq"
    with open(fq, "wb") as f:
        for i in range(len(lens)):
            s = bases[off[i]:off[i + 1]].tobytes()
            f.write(b"@q%d extra words\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    outs = {}
    # "workers": what a large input gets by default -- several workers with a one-lane workspace each, sized and warmed
    # before the queries (mtsv_batch_create_lanes / _reserve_host), taking groups of batches (here four of 10 000 reads);
    # "clean": the same with the orderly teardown instead of _exit
    many = {"MTSV_CLI_WORKERS": "3", "MTSV_CLI_GROUP_READS": "40000", "MTSV_HOST_THREADS": "6", "MTSV_INGEST_BLOCK": str(1 << 20)}
    for name, env, batch in (("serial", {"MTSV_SERIAL_INGEST": "1", "MTSV_HOST_THREADS": "1"}, "70000"),
                             ("par", {"MTSV_HOST_THREADS": "6", "MTSV_INGEST_BLOCK": str(1 << 20)}, "70000"),
                             ("workers", many, "10000"),
                             ("clean", dict(many, MTSV_CLI_CLEAN_EXIT="1", MTSV_CLI_TIMING="1", MTSV_CLI_MARKS="1"), "10000")):
        out = tmp_path / f"{name}.txt"
        r = subprocess.run([BIN, "--fastq", str(fq), "-i", str(idx), "-m", str(out), "--force-overwrite", "--batch-reads", batch],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout + r.stderr
        assert "threads terminated" in r.stdout
        outs[name] = open(out, "rb").read()
    assert outs["par"] == outs["serial"]
    assert outs["workers"] == outs["serial"] and outs["clean"] == outs["serial"]
    orc = O.Index.read(str(idx))
    hits, _ = orc.bin_batch(bases, off, O.default_params(), threads=8)
    want = set()
    cuts = np.flatnonzero(np.diff(hits["read"])) + 1          # hits are ordered by read
    for grp in np.split(hits, cuts):
        want.add(O.format_line(f"q{grp['read'][0]}", grp).rstrip("\n"))
    assert set(outs["par"].decode().splitlines()) == want
