"""CPU tests of the host-only side of the abundance step (mtsv_abundance_weights, mtsv_format_abundance, csrc/abund_rows.hpp)
against the plain-Python restatement in abund_ref.py, and of the restatement against the literals of the worked example in
include/mtsv_amd.h.  The device side is in test_abundance.py."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import abund_ref as A
import mtsv_tools_amd as M
import parse_cases as PC
import parse_ref as P
from mtsv_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "mtsv_amd.h")).read()
    for name in ("mtsv_fold_abundance", "mtsv_abundance_weights", "mtsv_format_abundance", "mtsv_abundance_row", "mtsv_abundance_info"):
        assert name in src
    for name in ("mtsv_fold_abundance", "mtsv_abundance_weights", "mtsv_format_abundance"):
        assert name in _lib.EXPORTS and hasattr(M.lib(), name)
    assert M.ABUNDANCE_ROW_DTYPE.itemsize == 40 and M.ABUNDANCE_ROW_DTYPE.fields["mass"][1] == 8
    import ctypes as C
    assert C.sizeof(M.AbundanceInfo) == 48 and M.AbundanceInfo.iterations.offset == 40 and M.AbundanceInfo.converged.offset == 44
    for name in ("abundance_weights", "format_abundance", "ABUNDANCE_ROW_DTYPE", "AbundanceInfo"):
        assert hasattr(M, name)
    assert hasattr(M.Fold, "abundance")


def test_the_restatement_gives_the_worked_example():
    w = A.weights(0.5, 64)
    assert w[:3] == [2 ** 31, 2 ** 30, 2 ** 29]
    for k in (1, 2, 3):
        r = A.run(A.EXAMPLE, w, slack=A.ALL, max_iters=k, tol=0)
        assert r["history"] == A.EXAMPLE_AFTER[:k]
        assert r["info"]["iterations"] == k and r["info"]["converged"] == 0 and r["info"]["l1_change"] == A.EXAMPLE_AFTER[k - 1][1]
    assert A.EXAMPLE_AFTER[2] == ({5: 8077478865, 7: 4807423021, 9: 4294967296}, 581047654)
    assert r["assigned"] == [(0, 5, 0), (1, 5, 1), (2, 7, 0), (3, 9, 3)] == A.EXAMPLE_ASSIGNED
    assert {t: (a, u, n) for t, _, a, u, n in r["rows"]} == {5: (3, 1, 2), 7: (2, 0, 1), 9: (1, 1, 1)} == A.EXAMPLE_ROWS_COUNTS
    assert r["info"] == dict(reads=4, entries=6, taxa=3, total_mass=17179869182, l1_change=581047654, iterations=3, converged=0)
    # no iteration: A stays A_0 and the assignment is by smallest edit, ties to the smallest TaxID
    r0 = A.run(A.EXAMPLE, w, max_iters=0)
    assert r0["assigned"] == A.EXAMPLE_ASSIGNED and r0["info"]["l1_change"] == 0 and [m for _, m, _, _, _ in r0["rows"]] == [2 ** 32] * 3


@pytest.mark.parametrize("n_w", [1, 64, 255])
@pytest.mark.parametrize("q", [1.0, 0.5, 0.25, 0.3, 1e-3, 1e-12])
def test_weights_against_the_restatement(q, n_w):
    got = M.abundance_weights(q, n_w)
    assert got.dtype == np.dtype("<u4") and got.tolist() == A.weights(q, n_w)
    if q == 0.5:
        assert got.tolist() == [2 ** (32 - d) if d <= 32 else 0 for d in range(1, n_w + 1)]
    if q == 1.0:
        assert got.tolist() == [2 ** 32 - 1] * n_w


@pytest.mark.parametrize("q", [0.0, -0.25, 1.0000001, 2.0, math.nan, math.inf])
def test_weights_refuse_q_outside_the_unit_interval(q):
    with pytest.raises(M.MtsvError) as e:
        M.abundance_weights(q, 8)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(ValueError):
        A.weights(q, 8)


@pytest.mark.parametrize("n_w", [0, 256])
def test_weights_refuse_a_table_outside_1_to_255(n_w):
    with pytest.raises(M.MtsvError) as e:
        M.abundance_weights(0.5, n_w)
    assert e.value.code == _lib.E_ARG


def rows_array(rows):
    a = np.zeros(len(rows), dtype=M.ABUNDANCE_ROW_DTYPE)
    for k, row in enumerate(rows):
        a[k] = row
    return a


def test_format_abundance_byte_for_byte():
    rng = random.Random(9)
    rows = [(t, rng.randrange(2 ** 40), rng.randrange(1000), rng.randrange(100), rng.randrange(500)) for t in sorted(rng.sample(range(2 ** 32), 300))]
    rows += [(2 ** 32 - 1, 2 ** 53 + 1, 2 ** 64 - 1, 0, 7)]
    rows[3] = (rows[3][0], 2 ** 62 + 12345, 5, 5, 5)                                # masses no double holds
    rows[4] = (rows[4][0], 2 ** 64 - 1, 1, 0, 0)
    rows[5] = (rows[5][0], 0, 0, 0, 0)
    for total in (sum(r[1] for r in rows) % 2 ** 64, 2 ** 63 + 1, 1, 0):
        want = A.tsv(rows, total)
        assert M.format_abundance(rows_array(rows), dict(total_mass=total)) == want
        assert want.startswith(A.HEADER.encode()) and want.count(b"\n") == len(rows) + 1
    # the worked example's table
    r = A.run(A.EXAMPLE, A.weights(0.5, 64), max_iters=3)
    text = M.format_abundance(rows_array(r["rows"]), r["info"])
    assert text == A.tsv(r["rows"], r["info"]["total_mass"])
    assert text.split(b"\n")[1] == b"5\t1.880685\t47.0171\t3\t1\t2"                 # 8077478865 / 2^32 and of 17179869182
    # an empty table: the header alone
    assert M.format_abundance(rows_array([]), dict(total_mass=0)) == A.HEADER.encode()


def test_abund_rows_under_the_sanitizers(tmp_path):
    """weights and formatter edge values as a stand-alone program built with the address and undefined-behaviour sanitizers
    and run on the CPU"""
    exe = tmp_path / "abund_rows_check"
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tools", "abund_rows_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "abund_rows_check ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_the_golden_results_converge_before_the_cap_at_the_cli_defaults():
    ids, recs = P.collapse_files(P.TAXID, [open(os.path.join(PC.GOLDEN, "e2e_default.results")).read()])
    assert len(ids) == 140 and len(recs) == 573 and max(len(per) for per in A.entries(recs, A.ALL).values()) == 8
    tol = int(math.floor(0.01 * 4294967296.0))
    r = A.run(recs, A.weights(0.25, 64), slack=A.ALL, max_iters=100, tol=tol)
    assert r["info"]["iterations"] == 19 and r["info"]["converged"] == 1
    assert r["info"]["l1_change"] == 31283348 <= tol
    assert r["info"]["reads"] == 140 and r["info"]["entries"] == 573
