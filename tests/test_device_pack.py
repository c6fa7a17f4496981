"""-m gpu: the index packed on the device at upload (MTSV_DEV_PACK_ON_DEVICE, k_pack.hip) and mtsv-binner --fold-prefetch.

Per rung of pack_ref.RUNG_NAMES the index is written to a file and loaded twice; one handle is uploaded with DEV_DEFAULT
(the host pack), the other with DEV_PACK_ON_DEVICE.  What is resident is read back with mtsv_index_download_device and
compared with pack_ref's restatement computed from the file's bytes (test_device_pack_cpu.py pins that restatement by
brute force) -- never with the other upload alone.  Then: the tile edges moved onto every block, hits and counters of the
device-packed index against the oracle, corrupted Occ checkpoints, and the command line."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import pack_ref as P
from mtsv_tools_amd import _lib
from oracle import oracle as O
from test_index_geometry import DENSE, SMALL_SEEDS, assert_counters, both_params, run, tiny_extras

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
PARTS = {"blocks": M.DEVPART_BLOCKS, "text": M.DEVPART_TEXT, "sa_sample": M.DEVPART_SA_SAMPLE, "bins": M.DEVPART_BINS,
         "bin_end": M.DEVPART_BIN_END, "bin_lut": M.DEVPART_BIN_LUT}
TIMES = ("pack_ms", "copy_ms", "accel_build_ms")
PACK = M.DEV_PACK_ON_DEVICE


class Written:
    """one rung built once: its file, the file as pack_ref reads it, and what pack_ref says the device must hold"""

    def __init__(self, rung, tmp):
        self.rung = rung
        self.entries = rung.entries()
        self.text = helpers.geometry_text(self.entries)
        self.path = str(tmp / (rung.name + ".idx"))
        ix = M.MGIndex.build(self.entries, rung.occ_k, rung.sa_s, threads=4)
        ix.write(self.path)
        ix.close()
        self.file = P.IndexFile(self.path)
        self.want = dict(P.small_parts(self.file), blocks=P.blocks(self.file.bwt), text=P.codes(self.file.text))
        self.header = P.header(self.file)
        self._orc = None

    @property
    def orc(self):
        if self._orc is None:
            self._orc = O.Index.read(self.path)
        return self._orc


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pack")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Written(helpers.RUNG_BY_NAME[name], tmp)
        return cache[name]

    return get


def resident(ix):
    h = ix.download_device(0, M.DEVPART_HEADER)
    return h, {name: ix.download_device(0, part) for name, part in PARTS.items()}


def check_against_restatement(w, ix, flags, packed):
    """every part and every scalar of the index resident behind ix, against pack_ref; returns (header, parts)"""
    h, parts = resident(ix)
    for name, want in w.want.items():
        got = parts[name]
        assert len(got) == len(want), (w.rung.name, name, len(got), len(want))
        if got != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"{w.rung.name} {name}: first differing byte {at} (block {at // 64}) of {len(want)}, packed_on_device={packed}")
    for key, want in w.header.items():
        assert h[key] == want, (w.rung.name, key, h[key], want)
    assert h["packed_on_device"] == packed
    assert h["kmer_k"] == (0 if flags & M.DEV_NO_KMER_TABLE else helpers.kmer_width_for(w.rung.n))
    assert h["sa_full"] == (0 if flags & M.DEV_SAMPLED_SA_ONLY else 1)
    info = ix.info()
    assert (info["kmer_k"], info["sa_full"], info["device_bytes"]) == (h["kmer_k"], h["sa_full"], h["device_bytes"])
    assert all(h[t] >= 0 for t in TIMES)
    return h, parts


def scalars(h):
    return {k: v for k, v in h.items() if k not in TIMES and k != "packed_on_device"}


# ---- 1. what is resident ----

@pytest.mark.parametrize("name", P.RUNG_NAMES)
def test_device_pack_leaves_the_host_packs_bytes(written, name):
    w = written(name)
    host, dev = M.MGIndex.load(w.path), M.MGIndex.load(w.path)
    try:
        host.to_device(0, M.DEV_DEFAULT)
        dev.to_device(0, PACK)
        hh, hp = check_against_restatement(w, host, 0, 0)
        dh, dp = check_against_restatement(w, dev, 0, 1)
        assert hp == dp and scalars(hh) == scalars(dh)
        assert host.info() == dev.info()
        print(f"{name}: host pack {hh['pack_ms']:.3f} copy {hh['copy_ms']:.3f} accel {hh['accel_build_ms']:.3f} ms; "
              f"device pack {dh['pack_ms']:.3f} copy {dh['copy_ms']:.3f} accel {dh['accel_build_ms']:.3f} ms")
    finally:
        host.close()
        dev.close()


def test_the_environment_switch_packs_on_the_device_without_the_flag(written, monkeypatch):
    w = written("random-8193")
    ix = M.MGIndex.load(w.path)
    try:
        monkeypatch.setenv("MTSV_DEV_PACK", "device")
        ix.to_device(0, M.DEV_DEFAULT)
        check_against_restatement(w, ix, 0, 1)
        monkeypatch.setenv("MTSV_DEV_PACK", "host")           # (anything but "device" is the default; read at every upload)
        ix.to_device(0, M.DEV_NO_KMER_TABLE)
        check_against_restatement(w, ix, M.DEV_NO_KMER_TABLE, 0)
        monkeypatch.delenv("MTSV_DEV_PACK")
        ix.to_device(0, M.DEV_DEFAULT)
        check_against_restatement(w, ix, 0, 0)
    finally:
        ix.close()


# ---- 2. a tile edge at every block, at every second block ----

@pytest.mark.parametrize("tile", ["1", "2"])
@pytest.mark.parametrize("name", [n for n in P.RUNG_NAMES if helpers.RUNG_BY_NAME[n].n <= 8193])
def test_tile_edges_at_every_block(written, name, tile, monkeypatch):
    w = written(name)
    ix = M.MGIndex.load(w.path)
    try:
        monkeypatch.setenv("MTSV_PACK_TILE", tile)
        ix.to_device(0, PACK)
        check_against_restatement(w, ix, 0, 1)
    finally:
        ix.close()


def traced_tiles(capfd):
    """the tiles of the device packs traced since the last look"""
    return re.findall(r"\[upload\] pack on device, tile (\d+):", capfd.readouterr().err)


@pytest.mark.parametrize("tile", ["4", "8", "16", "32"])
def test_tiles_between_two_blocks_and_the_default(written, tile, monkeypatch, capfd):
    w = written("random-8193")                                                     # 65 blocks: 17, 9, 5 and 3 tiles, the last of one block
    ix = M.MGIndex.load(w.path)
    try:
        monkeypatch.setenv("MTSV_PACK_TILE", tile)
        monkeypatch.setenv("MTSV_TRACE", "1")
        ix.to_device(0, PACK)
        h, _ = check_against_restatement(w, ix, 0, 1)
        assert h["n_blocks"] == 65 and traced_tiles(capfd) == [tile]
    finally:
        ix.close()


# ---- 2b. the carry of k_pack_scan: one workgroup walks PACK_ROUND tiles per round and carries their sums into the next ----

PACK_ROUND = 1024
# (rung, tile, rounds, tiles of the last round): random-524161 has 4096 blocks, random-131073 has 1025 -- a second round of one
# tile behind a full one.  The rounds are asserted from the resident header's n_blocks, not from the rung's name.
CARRY_CASES = [("random-524161", 4, 1, 1024), ("random-524161", 2, 2, 1024), ("random-524161", 1, 4, 1024), ("random-131073", 1, 2, 1)]


@pytest.mark.parametrize("name,tile,n_rounds,last", CARRY_CASES, ids=[f"{c[0]}-tile{c[1]}" for c in CARRY_CASES])
def test_scan_carry_over_rounds_of_1024_tiles(written, name, tile, n_rounds, last, monkeypatch, capfd):
    w = written(name)
    ix = M.MGIndex.load(w.path)
    try:
        monkeypatch.setenv("MTSV_PACK_TILE", str(tile))
        monkeypatch.setenv("MTSV_TRACE", "1")
        ix.to_device(0, PACK)
        h, _ = check_against_restatement(w, ix, 0, 1)
        assert traced_tiles(capfd) == [str(tile)]
        tiles = -(-h["n_blocks"] // tile)
        assert (-(-tiles // PACK_ROUND), tiles - (n_rounds - 1) * PACK_ROUND) == (n_rounds, last)
    finally:
        ix.close()


# ---- 3. what is built on the device-packed blocks: the full suffix array, the table, its levels and tags ----

@pytest.mark.parametrize("name", ["random-129", "random-8193", "sentinel-res0", "nrun-20000", "ACG-4096"])
def test_hits_of_the_device_packed_index_equal_the_oracles(written, name):
    w = written(name)
    rng = random.Random(w.rung.n)
    probes = [r for _, r in helpers.position_probes(w.text)]
    cases = [(probes, dict(edit_rate=0.0), 0)]
    if w.rung.n < 257:
        cases.append((tiny_extras(rng, w.text), dict(edit_rate=0.0), 0))
        small = [r for _, r in helpers.position_probes(w.text, width=8)] + tiny_extras(rng, w.text)
        cases += [(small, over, 0) for over in SMALL_SEEDS]
    if name == "ACG-4096":
        cases.append((probes, DENSE, 4_000_000))
    wants = []
    for reads, over, ws in cases:
        mp, op = both_params(**over)
        bases, off = helpers.reads_to_batch(reads)
        wants.append((reads, mp, ws, over) + w.orc.bin_batch(bases, off, op, threads=8))
    assert sum(c["H"] for *_, c in wants) > 0
    ix = M.MGIndex.load(w.path)
    try:
        for older in (M.DEV_SAMPLED_SA_ONLY | M.DEV_NO_KMER_TABLE, M.DEV_SAMPLED_SA_ONLY, M.DEV_NO_KMER_TABLE, M.DEV_DEFAULT):
            ix.to_device(0, older | PACK)
            h = ix.download_device(0, M.DEVPART_HEADER)
            assert h["packed_on_device"] == 1 and h["sa_full"] == (0 if older & M.DEV_SAMPLED_SA_ONLY else 1)
            assert h["kmer_k"] == (0 if older & M.DEV_NO_KMER_TABLE else helpers.kmer_width_for(w.rung.n))
            for reads, mp, ws, over, want, ctr in wants:
                got, st = run(ix, reads, mp, 0, ws)
                helpers.assert_same_hits(got, want)
                assert_counters(st, ctr, not older & M.DEV_SAMPLED_SA_ONLY, (name, older | PACK, over))
    finally:
        ix.close()


# ---- 4. a file whose Occ table disagrees with its bwt ----

def patched(w, tmp_path, tag, patches):
    """the rung's file with the u64 occ[sym][j] changed (0 becomes 1, any other value one less) for every (sym, j) of patches"""
    raw = bytearray(open(w.path, "rb").read())
    for sym, j in patches:
        at = w.file.occ_offset(sym, j)
        v = int.from_bytes(raw[at:at + 8], "little")
        assert v == w.file.occ[sym][j]
        raw[at:at + 8] = (v + 1 if v == 0 else v - 1).to_bytes(8, "little")
    p = str(tmp_path / (tag + ".idx"))
    open(p, "wb").write(bytes(raw))
    return p


def upload_error(path, flags):
    ix = M.MGIndex.load(path)      # (the loader checks the file's structure, not its Occ values)
    try:
        with pytest.raises(M.MtsvError) as e:
            ix.to_device(0, flags)
        assert e.value.code == _lib.E_FORMAT
        assert ix.info()["device_bytes"] == 0
        with pytest.raises(M.MtsvError) as e2:  # nothing is resident after the failure
            ix.download_device(0, M.DEVPART_HEADER)
        assert e2.value.code == _lib.E_ARG
        return str(e.value)
    finally:
        ix.close()


def test_occ_corruption_is_reported_alike_by_both_packs(written, tmp_path):
    w = written("random-8193")
    f = w.file
    n_chk = (f.n - 1) // f.k + 1
    assert n_chk == 129 and all(len(f.occ[s]) == n_chk for s in P.SYMS)
    srow = w.header["sentinel_row"]
    assert f.k <= srow < (n_chk - 1) * f.k                           # a checkpoint before it and one behind it
    j1, j0 = 77, 5
    before, behind = (srow - 1) // f.k, (srow + f.k - 1) // f.k
    assert before * f.k < srow <= behind * f.k and f.occ["$"][before] == 0 and f.occ["$"][behind] == 1
    cases = {"g": ([("G", j1)], j1), "g_and_n": ([("G", j1), ("N", j0)], j0), "last": ([("T", n_chk - 1)], n_chk - 1), "first": ([("A", 0)], 0),
             "sentinel_before": ([("$", before)], before), "sentinel_behind": ([("$", behind)], behind)}
    for tag, (patches, first_bad) in cases.items():
        p = patched(w, tmp_path, tag, patches)
        msgs = [upload_error(p, flags) for flags in (M.DEV_DEFAULT, PACK, PACK | M.DEV_SAMPLED_SA_ONLY | M.DEV_NO_KMER_TABLE)]
        assert msgs[0] == msgs[1] == msgs[2], (tag, msgs)
        assert msgs[0].endswith(f"format: Occ checkpoint {first_bad} disagrees with the bwt"), (tag, msgs[0])
    # a handle that failed on the device pack is uploaded from the good file's bytes afterwards: same process, same device
    for flags in (PACK, M.DEV_DEFAULT):
        ix = M.MGIndex.load(w.path)
        try:
            ix.to_device(0, flags)
            check_against_restatement(w, ix, 0, 1 if flags & PACK else 0)
        finally:
            ix.close()


# ---- 5. the command line ----

def run_binner(*args, env=None):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})


OUT_NAMES = ("res.txt", "rep.tsv", "m.fq", "u.fq")


def outputs(d, tag):
    return [d / (tag + "_" + n) for n in OUT_NAMES]


def binner_run(fx, tag, switches, env=None, index=None):
    res, rep, m, u = outputs(fx["dir"], tag)
    r = run_binner("--fastq", fx["fq"], "-i", index or fx["index"], "-m", res, "--report", rep, "--matched", m, "--unmatched", u, *switches,
                   env={"MTSV_CLI_TIMING": "1", **(env or {})})
    return r, [res, rep, m, u]


@pytest.fixture(scope="module")
def chunks3(tmp_path_factory):
    """three chunks of 24 000 symbols, 2 800 reads of 100 bases: 800 drawn from each chunk and 400 from none; the
    reference files of --merge-on-gpu and of --fold-on-gpu without the prefetch, in both formats"""
    d = tmp_path_factory.mktemp("prefetch_cli")
    paths, rows = [], []
    for c in range(3):
        ix = M.MGIndex.synth(seed=31 + c, n_taxa=6, gis_per_taxon=2, seq_len=2000)
        p = str(d / f"chunk{c}.idx")
        ix.write(p)
        paths.append(p)
        bases, _ = M.synth_reads(ix, seed=41 + c, n_reads=800, read_len=100)
        rows.append(np.asarray(bases).reshape(-1, 100))
        ix.close()
    rng = random.Random(5)
    rows.append(np.frombuffer(helpers.rnd_seq(rng, 400 * 100), dtype=np.uint8).reshape(-1, 100))
    reads = np.concatenate(rows)
    reads = reads[np.random.default_rng(7).permutation(len(reads))]
    fq = d / "reads.fastq"
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * 100))
    fx = {"dir": d, "fq": fq, "index": ",".join(paths), "paths": paths, "n": len(reads), "ref": {}}
    for fmt, extra in (("default", []), ("long", ["--output-format", "long"])):
        r, merged = binner_run(fx, "merge_" + fmt, ["--merge-on-gpu", *extra])
        assert r.returncode == 0, r.stdout + r.stderr
        r, folded = binner_run(fx, "fold_" + fmt, ["--fold-on-gpu", "--fold-reads", "1000", *extra])
        assert r.returncode == 0, r.stdout + r.stderr
        t = re.search(r"\[cli fold timing\] super_batches (\d+) chunks (\d+) reads (\d+)", r.stderr)
        assert t and int(t.group(1)) >= 3 and (int(t.group(2)), int(t.group(3))) == (3, len(reads)) and "prefetch" not in r.stderr
        for a, b in zip(merged, folded):
            assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 0
        assert 0 < merged[3].read_bytes().count(b"\n+\n") < len(reads)      # some reads match, some do not
        fx["ref"][fmt] = [x.read_bytes() for x in merged]
    return fx


PREFETCH_CASES = {
    "default": ([], {}, "default"),
    "long": (["--output-format", "long"], {}, "long"),
    "default_pack_on_device": ([], {"MTSV_DEV_PACK": "device"}, "default"),
    "long_pack_on_device": (["--output-format", "long"], {"MTSV_DEV_PACK": "device"}, "long"),
    "text_on_gpu": (["--text-on-gpu"], {}, "default"),
    "text_on_gpu_clean_exit": (["--text-on-gpu"], {"MTSV_CLI_CLEAN_EXIT": "1", "MTSV_DEV_PACK": "device"}, "default"),
}


@pytest.mark.parametrize("case", list(PREFETCH_CASES))
def test_binner_fold_prefetch_writes_the_same_files(chunks3, case):
    extra, env, fmt = PREFETCH_CASES[case]
    r, got = binner_run(chunks3, "pre_" + case, ["--fold-on-gpu", "--fold-prefetch", "--fold-reads", "1000", *extra], env)
    assert r.returncode == 0, r.stdout + r.stderr
    t = re.search(r"\[cli fold timing\] super_batches (\d+) chunks 3 reads (\d+);.*prefetch: loader ([0-9.]+) s, waited_for_loader ([0-9.]+) s", r.stderr)
    assert t and int(t.group(1)) >= 3 and int(t.group(2)) == chunks3["n"], r.stderr
    for path, want in zip(got, chunks3["ref"][fmt]):
        assert path.read_bytes() == want, path


def test_a_chunk_that_fails_to_load_is_reported_when_its_turn_comes(chunks3):
    missing = str(chunks3["dir"] / "no_such_chunk.idx")
    index = ",".join([chunks3["paths"][0], missing, chunks3["paths"][2]])
    seen = []
    for tag, switches, env in (("miss_plain", [], {}), ("miss_pre", ["--fold-prefetch"], {}), ("miss_pre_clean", ["--fold-prefetch"], {"MTSV_CLI_CLEAN_EXIT": "1"})):
        r, _ = binner_run(chunks3, tag, ["--fold-on-gpu", "--fold-reads", "1000", *switches], env, index=index)
        assert r.returncode == 2, r.stdout + r.stderr
        lines = [ln.split("Error running query: ", 1)[1] for ln in (r.stdout + r.stderr).splitlines() if "Error running query: " in ln]
        assert len(lines) == 1 and missing in lines[0] and lines[0].startswith("io:"), r.stdout + r.stderr
        seen.append(lines[0])
    assert seen[0] == seen[1] == seen[2]
