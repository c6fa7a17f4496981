"""What of the dedup step needs no GPU: the restatement (dedup_ref.py) on a hand-written case, the library's exports and
their refusal of NULL handles, and the argument rule of mtsv-binner --dedup, which is decided before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import dedup_ref as D
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
DEDUP_SYMBOLS = ("mtsv_dupmap_create", "mtsv_dupmap_free", "mtsv_batch_take_unique", "mtsv_dupmap_download", "mtsv_fold_expand")


def test_restatement_on_a_hand_written_case():
    raw = [b"ACGT", b"acgt", b"ACGTA", b"ACG", b"ACGN", b"ACGR", b"TCGT", b"", b"ACGT", b"", b"ACGA"]
    bases = np.frombuffer(b"".join(raw), dtype=np.uint8)
    off = np.cumsum([0] + [len(r) for r in raw]).astype(np.uint64)
    reads = D.read_codes(bases, off)
    assert reads[0] == bytes([0, 1, 2, 3]) and reads[4] == reads[5] == bytes([0, 1, 2, 4])
    # case and the letter that stands for N collapse; a prefix, a longer read and a changed first or last base do not
    assert D.rep(reads) == [0, 0, 2, 3, 4, 4, 6, 7, 0, 7, 10]
    assert D.representatives(reads) == [0, 2, 3, 4, 6, 7, 10]
    read, rep = D.dupmap(reads, src_map=[10 * j + 3 for j in range(len(raw))])
    assert read == [3, 13, 23, 33, 43, 53, 63, 73, 83, 93, 103] and rep == [3, 3, 23, 33, 43, 43, 63, 73, 3, 73, 103]
    # the fan: records of the representatives 0 and 4 (none for 2), under every read they stand for, in read order
    recs = [(0, 7, 1), (0, 9, 0), (4, 7, 5)]
    read, rep = D.dupmap(reads)
    assert D.expand(recs, read, rep) == [(0, 7, 1), (0, 9, 0), (1, 7, 1), (1, 9, 0), (4, 7, 5), (5, 7, 5), (8, 7, 1), (8, 9, 0)]
    wide = [(0, 7, 2, 30, 1), (4, 7, 2, 31, 5)]
    assert D.expand(wide, read, rep)[1] == (1, 7, 2, 30, 1) and len(D.expand(wide, read, rep)) == 5
    assert D.expand([], read, rep) == [] and D.dupmap([]) == ([], [])


def test_library_exports_every_dedup_symbol_and_refuses_null_handles():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.lib_path())
    for name in DEDUP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert "typedef struct mtsv_dupmap mtsv_dupmap;" in src and hasattr(M, "DupMap")
    L = M.lib()
    p, q, n, u, ms = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_float()
    assert L.mtsv_dupmap_create(0, None) == _lib.E_ARG
    assert L.mtsv_batch_take_unique(None, None, None, C.byref(n), C.byref(u), C.byref(ms)) == _lib.E_ARG
    assert L.mtsv_dupmap_download(None, C.byref(p), C.byref(q), C.byref(n), C.byref(u)) == _lib.E_ARG
    assert L.mtsv_fold_expand(None, None, None, C.byref(ms)) == _lib.E_ARG
    assert b"null" in L.mtsv_last_error()
    L.mtsv_dupmap_free(None)                                                   # like free(NULL)


def binner(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_help_lists_the_switch():
    assert "--dedup" in binner("--help").stdout


def test_dedup_without_fold_on_gpu_is_a_usage_error(tmp_path):
    """the index files do not exist: a run that got as far as loading one would exit 2"""
    res, fq = tmp_path / "res", tmp_path / "x.fastq"
    two = f"{tmp_path}/a.idx,{tmp_path}/b.idx"
    for other in ([], ["--merge-on-gpu"]):
        r = binner("--fastq", fq, "-i", two, "-m", res, "--dedup", *other)
        assert r.returncode == 1 and "The argument '--dedup' requires '--fold-on-gpu'" in r.stderr, r.stderr
    assert not res.exists()
    # with the switch it belongs to, the run gets as far as its input
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--dedup")
    assert r.returncode == 2, r.stderr
