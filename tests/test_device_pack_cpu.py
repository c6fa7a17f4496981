"""CPU tests for the device-side pack (k_pack.hip): the restatement the GPU tests compare with is pinned by brute force on
every rung they use, the library exports the new call and flag, and mtsv-binner decides the rule of --fold-prefetch
before it opens anything."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
import mtsv_tools_amd as M
import pack_ref as P
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def test_the_rungs_exist_and_sit_where_they_claim():
    rungs = [helpers.RUNG_BY_NAME[n] for n in P.RUNG_NAMES]
    assert len(rungs) == 28 and max(r.n for r in rungs) == 524161
    assert {(r.occ_k, r.sa_s) for r in rungs} >= {(64, 32), (3, 5), (128, 7), (1, 1), (262, 258), (4102, 32)}
    assert any(r.n % 128 == 0 for r in rungs) and any(r.n % 8192 == 1 for r in rungs)


@pytest.mark.parametrize("name", P.RUNG_NAMES)
def test_restated_blocks_answer_every_rank_query_by_brute_force(name, tmp_path):
    """rank(a, i) for every row i in 0..n and every symbol, read from pack_ref.blocks the way the kernels read it (cnt +
    the rows of the block before i; N derived from the rows before the block, the four counts and the sentinel's row),
    equals a plain count over the bwt bytes of the file"""
    rung = helpers.RUNG_BY_NAME[name]
    path = str(tmp_path / "x.idx")
    ix = M.MGIndex.build(rung.entries(), rung.occ_k, rung.sa_s, threads=4)
    ix.write(path)
    ix.close()
    f = P.IndexFile(path)
    n = f.n
    assert n == rung.n and f.k == rung.occ_k and f.s == rung.sa_s
    raw = P.blocks(f.bwt)
    nb = (n >> 7) + 1
    assert len(raw) == 64 * nb
    blk = np.frombuffer(raw, dtype=np.dtype([("cnt", "<u4", 4), ("p", "<u8", (3, 2))]))
    bits = np.unpackbits(blk["p"].copy().view(np.uint8).reshape(nb, 3, 16), axis=2, bitorder="little")  # [block, plane, row]
    code = (bits[:, 0] | bits[:, 1] << 1 | bits[:, 2] << 2).reshape(-1)
    bwt = np.frombuffer(f.bwt, dtype=np.uint8)
    want_code = np.full(256, 7, dtype=np.uint8)
    for c, v in P.CODE.items():
        want_code[c] = v
    assert np.array_equal(code[:n], want_code[bwt]) and np.all(code[n:] == 7) and len(code) == nb * 128 > n
    srow = int(np.flatnonzero(bwt == ord("$"))[0])
    assert P.header(f)["sentinel_row"] == srow and (bwt == ord("$")).sum() == 1
    i = np.arange(n + 1)
    b, off = i >> 7, i & 127
    for a, sym in enumerate(b"ACGTN"):
        brute = np.concatenate(([0], np.cumsum(bwt == sym)))                      # brute[i] = occurrences in bwt[0 .. i)
        eq = (code == a).reshape(nb, 128)
        within = np.concatenate((np.zeros((nb, 1), dtype=np.int64), np.cumsum(eq, axis=1)), axis=1)[b, off]
        if a < 4:
            base = blk["cnt"][b, a].astype(np.int64)
        else:
            before = b.astype(np.int64) << 7
            base = before - blk["cnt"][b].astype(np.int64).sum(axis=1) - (before > srow)
        assert np.array_equal(base + within, brute), (name, chr(sym))
    # the file's own checkpoints agree with the same count: what the upload's cross-check relies on
    for a, sym in enumerate(P.SYMS):
        brute = np.cumsum(bwt == ord(sym))
        assert f.occ[sym] == [int(brute[j * f.k]) for j in range((n - 1) // f.k + 1)]
        at = f.occ_offset(sym, len(f.occ[sym]) - 1)
        assert int.from_bytes(open(path, "rb").read()[at:at + 8], "little") == f.occ[sym][-1]
    assert P.codes(f.text)[:n] == bytes(want_code[np.frombuffer(f.text, dtype=np.uint8)]) and len(P.codes(f.text)) == (n + 15) // 16 * 16 + 32


def test_library_exports_the_download_and_the_flag():
    lib = ctypes.CDLL(M.lib_path())
    assert hasattr(lib, "mtsv_index_download_device") and "mtsv_index_download_device" in _lib.EXPORTS
    assert M.DEV_PACK_ON_DEVICE == 4
    assert ctypes.sizeof(M.DeviceHeader) == 88
    assert (M.DEVPART_HEADER, M.DEVPART_BLOCKS, M.DEVPART_TEXT, M.DEVPART_SA_SAMPLE, M.DEVPART_BINS, M.DEVPART_BIN_END, M.DEVPART_BIN_LUT) == tuple(range(7))
    # not resident anywhere: an argument error, whatever the part
    ix = M.MGIndex.build([(1, 10, b"ACGTACGTAACCGGTTACGATCGATCGATCGTAGC")], threads=1)
    for part in (M.DEVPART_HEADER, M.DEVPART_BLOCKS, 99):
        with pytest.raises(M.MtsvError) as e:
            ix.download_device(0, part)
        assert e.value.code == _lib.E_ARG
    ix.close()


def binner(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_fold_prefetch_requires_fold_on_gpu_and_is_decided_before_any_index_is_opened(tmp_path):
    """every run names index files that do not exist: a run that got as far as loading one would exit 2"""
    res, fq = tmp_path / "res", tmp_path / "x.fastq"
    two = f"{tmp_path}/a.idx,{tmp_path}/b.idx"
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-prefetch")
    assert r.returncode == 1 and "--fold-prefetch" in r.stderr and "--fold-on-gpu" in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-prefetch", "--merge-on-gpu")
    assert r.returncode == 1 and "--fold-prefetch" in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", tmp_path / "a.idx", "-m", res, "--fold-prefetch")
    assert r.returncode == 1 and "--fold-prefetch" in r.stderr, r.stderr
    assert not res.exists()
    # with --fold-on-gpu the flag is accepted: the run gets as far as its input
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--fold-prefetch")
    assert r.returncode == 2, r.stderr
    assert "--fold-prefetch" in binner("--help").stdout
