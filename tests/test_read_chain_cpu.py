"""Chaining workspaces without a GPU: the numpy restatement of the compaction (chain_ref.py) on hand-made cases, the new
symbols of the library and their NULL checks, and the usage errors of mtsv-binner --filter-index, which are reached before
any file or device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np

import chain_ref as CR
import mtsv_tools_amd as M
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")


def batch(reads):
    codes = np.frombuffer(b"".join(reads), dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return codes, off


def test_normalise_is_the_binners_table():
    got = CR.normalise(np.frombuffer(b"ACGTacgtNnRY-*\x00\xff", dtype=np.uint8))
    assert got.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4]


def test_compact_on_hand_made_batches():
    reads = [b"\x00\x01", b"", b"\x02\x03\x04", b"\x01", b"", b"\x03\x03\x03\x03\x00"]
    codes, off = batch(reads)
    keep = [True, True, False, True, False, True]
    c, o, m = CR.compact(codes, off, keep)
    assert c.tolist() == [0, 1, 1, 3, 3, 3, 3, 0]
    assert o.tolist() == [0, 2, 2, 3, 8]                    # the empty read keeps its slot
    assert m.tolist() == [0, 1, 3, 5]
    assert o.dtype == np.uint64 and m.dtype == np.uint64 and c.dtype == np.uint8
    # nothing kept, everything kept
    c, o, m = CR.compact(codes, off, [False] * 6)
    assert len(c) == 0 and o.tolist() == [0] and len(m) == 0
    c, o, m = CR.compact(codes, off, [True] * 6)
    assert np.array_equal(c, codes) and np.array_equal(o, off) and m.tolist() == list(range(6))
    # offsets that do not start at 0 (a slice of a larger batch)
    c, o, m = CR.compact(codes, off[2:], [True, False, False, True])
    assert c.tolist() == [2, 3, 4, 3, 3, 3, 3, 0] and o.tolist() == [0, 3, 8] and m.tolist() == [0, 3]
    # no reads at all
    c, o, m = CR.compact(np.zeros(0, np.uint8), np.zeros(1, np.uint64), [])
    assert len(c) == 0 and o.tolist() == [0] and len(m) == 0


def test_maps_compose_along_a_chain():
    reads = [bytes([k % 5]) * (k % 4) for k in range(20)]
    codes, off = batch(reads)
    keep1 = np.array([k % 3 != 0 for k in range(20)])
    c1, o1, m1 = CR.compact(codes, off, keep1)
    keep2 = np.array([j % 2 == 1 for j in range(len(m1))])
    # the second step on the first's output, with the first's map handed in ...
    c2, o2, m2 = CR.compact(c1, o1, keep2, src_map=m1)
    # ... is the one step with both masks, and its map is the composition
    both = np.zeros(20, dtype=bool)
    both[m1[keep2].astype(np.int64)] = True
    c3, o3, m3 = CR.compact(codes, off, both)
    assert np.array_equal(c2, c3) and np.array_equal(o2, o3) and np.array_equal(m2, m3)
    _, _, own = CR.compact(c1, o1, keep2)
    assert np.array_equal(CR.compose(m1, own), m2)
    assert np.all(np.diff(m2.astype(np.int64)) > 0)          # maps ascend: hits stay ordered by original read
    assert np.array_equal(CR.keep_mask([True, False], False), [False, True])
    assert np.array_equal(CR.keep_mask([True, False], True), [True, False])


def test_the_new_symbols_exist_and_reject_null_handles():
    L = M.lib()
    assert (M.KEEP_UNMATCHED, M.KEEP_MATCHED) == (0, 1)
    for name in ("mtsv_batch_take_reads", "mtsv_batch_read_map", "mtsv_batch_download_reads"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    n, nb, ms, p, q = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_void_p(), C.c_void_p()
    assert L.mtsv_batch_take_reads(None, None, 0, C.byref(n), C.byref(nb), C.byref(ms)) == _lib.E_ARG
    assert b"null" in L.mtsv_last_error()
    assert L.mtsv_batch_read_map(None, C.byref(p), C.byref(n)) == _lib.E_ARG
    assert L.mtsv_batch_download_reads(None, C.byref(p), C.byref(q), C.byref(n)) == _lib.E_ARG
    header = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    assert "#define MTSV_KEEP_UNMATCHED 0" in header and "#define MTSV_KEEP_MATCHED 1" in header


def run(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_cli_refuses_what_the_chain_does_not_do_yet(tmp_path):
    res = tmp_path / "r"
    base = ("--fasta", "x", "-i", "y", "-m", res, "--filter-index", "f")
    for extra in (("--matched", tmp_path / "m"), ("--unmatched", tmp_path / "u"), ("--matched", tmp_path / "m", "--unmatched", tmp_path / "u")):
        r = run(*base, *extra)
        assert r.returncode == 1 and "--filter-index" in r.stderr and "cannot be used with" in r.stderr
    r = run("--fasta", "x", "--filter-index", "f", "--parse-only")
    assert r.returncode == 1 and "--parse-only" in r.stderr and "--filter-index" in r.stderr
    r = run("--fasta", "x", "-i", "a,b", "-m", res, "--filter-index", "f")
    assert r.returncode == 1 and "--filter-index" in r.stderr and "index chunks" in r.stderr
    r = run("--fasta", "x", "-i", "y", "-m", res, "--filter-index")
    assert r.returncode == 1 and "requires a value" in r.stderr
    assert not os.listdir(tmp_path)                          # nothing was created
    assert "--filter-index" in run("--help").stdout
    # the option itself is accepted: the run gets as far as opening its input
    assert run("--fasta", tmp_path / "missing.fa", "-i", "y", "-m", res, "--filter-index", "f").returncode == 2
