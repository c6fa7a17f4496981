"""CPU tests for the result lines written on the device (k_text.hip): the synthetic cases hold what they claim, the
restatement they are checked against equals the host formatters on them, the library exports the new calls, and
mtsv-binner decides the rules of --text-on-gpu before it opens anything."""
import ctypes
import os
import re
import subprocess

import numpy as np

import assign_ref as A
import fold_ref as F
import grain_ref as GR
import mtsv_tools_amd as M
import text_cases as T
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINNER = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-binner")
TEXT_SYMBOLS = ("mtsv_fold_format_text", "mtsv_batch_format_text")


def test_cases_hold_what_they_claim():
    assert T.LADDER[0] == 0 and T.LADDER[-1] == 4294967295 and sum(v >= 1 << 31 for v in T.LADDER) == 3
    for k in range(1, 10):
        assert 10 ** k in T.LADDER and 10 ** k - 1 in T.LADDER
    for grain in T.GRAINS.values():
        cases = T.cases(grain)
        for name, c in cases.items():
            assert F.is_list(grain, c.records) and F.is_list(grain, c.second), name
            blob, off = c.table
            n_reads = len(c.ids)
            assert len(off) == n_reads + 1 and off[0] == 0 and off[-1] == len(blob) and np.all(np.diff(off.astype(np.int64)) >= 0)
            assert all(r[0] < n_reads for r in c.records + c.second)
            for i, s in enumerate(c.ids):                                     # strnlen within the slot is the ID
                slot = blob[int(off[i]):int(off[i + 1])]
                assert slot.split(b"\0")[0] == s.encode() and set(slot[len(s):]) <= {0}, (name, i)
            have = {r[0] for r in c.records}
            want = T.expected(grain, c)
            assert b"ABSENT" not in want and want.count(b"\n") == len(have)
            if c.records:
                assert c.records[-1][0] == max(have) and want.endswith(b"\n")
        lad = cases["ladder"]
        fields = range(1, 3) if grain == F.TAXID else range(1, 5)
        for f in fields:                                                      # every field at every power of ten, and beyond bit 31
            vals = {r[f] for c in cases.values() for r in c.records}
            assert set(T.LADDER) <= vals, f
        have = sorted({r[0] for r in lad.records})
        assert tuple(len(lad.ids[r]) for r in have) == T.ID_LENGTHS
        assert have[-1] - have[0] + 1 > len(have) and len(lad.ids) > have[-1] + 1   # reads without records between and behind
        slots = {"pad" if sl.endswith(b"\0\0") else "nul" if sl.endswith(b"\0") else "full"
                 for c in cases.values() for sl in (c.table[0][int(c.table[1][i]):int(c.table[1][i + 1])] for i in range(len(c.ids)))}
        assert slots == {"nul", "pad", "full"}
        for n in (0, 1, 63, 64, 65, 197):
            assert len(cases[f"size_{n}"].records) == n
        c = cases["head_at_64"]
        assert c.records[63][0] != c.records[64][0] and len(c.records) > 64
        c = cases["straddle_63_64"]
        assert c.records[60][0] == c.records[63][0] == c.records[64][0] == c.records[70][0] != c.records[59][0]
        c = cases["one_read_of_six_tiles"]
        assert {r[0] for r in c.records} == {1} and len(c.records) > 5 * T.TILE
        # tile edges on every byte of a dword (and on most bytes of a 16-byte store), tile texts of every length mod 4
        edges = [e for c in cases.values() for e in T.tile_edges(grain, c)[1:-1]]
        assert {e % 4 for e in edges} == {0, 1, 2, 3} and len({e % 16 for e in edges}) >= 12
        lens = [b - a for c in cases.values() for a, b in zip(T.tile_edges(grain, c), T.tile_edges(grain, c)[1:])]
        assert {n % 4 for n in lens} == {0, 1, 2, 3}
        # more text in one default tile than two LDS windows of 32 KiB, and an ID longer than a window of 64-record tiles
        c = cases["many_long_ids"]
        e = T.tile_edges(grain, c, 1024)
        assert e[1] - e[0] > 2 * 32768 and max(len(s) for s in lad.ids) > 2 * 32 * T.TILE


def test_restatement_equals_the_host_formatters():
    for grain in T.GRAINS.values():
        for name, c in T.cases(grain).items():
            for recs in (c.records, F.fold(grain, c.records, c.second)):
                want = T.text(grain, recs, c.ids)
                assert T.host_format(grain, recs, c.table) == want, name        # NUL-padded and unterminated slots
                if grain == F.TAXID:
                    got = M.format_assignments(A.as_array(recs, M.ASSIGN_DTYPE), c.ids)
                else:
                    got = M.format_assignments_gi(GR.as_array(recs, M.ASSIGN_GI_DTYPE), c.ids)
                assert got.encode() == want, name


def test_library_exports_the_text_calls():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.lib_path())
    for name in TEXT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert callable(M.Fold.format_text) and callable(M.Batch.format_text)


def test_null_arguments_are_argument_errors():
    L = _lib.lib()
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    off = np.zeros(1, dtype=np.uint64)
    for call in (L.mtsv_fold_format_text, L.mtsv_batch_format_text):
        assert call(None, b"", off.ctypes.data, 0, ctypes.byref(out), ctypes.byref(n), None) == _lib.E_ARG


def binner(*args):
    return subprocess.run([BINNER, *map(str, args)], capture_output=True, text=True, timeout=120)


def test_text_on_gpu_argument_rules_are_decided_before_any_index_is_opened(tmp_path):
    """every run names index files that do not exist: a run that got as far as loading one would exit 2"""
    res, fq = tmp_path / "res", tmp_path / "x.fastq"
    two = f"{tmp_path}/a.idx,{tmp_path}/b.idx"
    r = binner("--fastq", fq, "-i", two, "-m", res, "--text-on-gpu")
    assert r.returncode == 1 and "--text-on-gpu" in r.stderr and "--fold-on-gpu" in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", tmp_path / "a.idx", "-m", res, "--text-on-gpu")
    assert r.returncode == 1 and "--text-on-gpu" in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--text-on-gpu", "--merge-on-gpu")
    assert r.returncode == 1 and "--text-on-gpu" in r.stderr and "--merge-on-gpu" in r.stderr, r.stderr
    r = binner("--fastq", fq, "-i", two, "-m", res, "--merge-on-gpu", "--text-on-gpu", "--fold-on-gpu")
    assert r.returncode == 1, r.stderr
    assert not res.exists()
    # with --fold-on-gpu the flag is accepted: the run gets as far as its input
    r = binner("--fastq", fq, "-i", two, "-m", res, "--fold-on-gpu", "--text-on-gpu")
    assert r.returncode == 2, r.stderr
    assert "--text-on-gpu" in binner("--help").stdout
