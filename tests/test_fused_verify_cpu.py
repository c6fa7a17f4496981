"""The three facts the fused verify pass (k_edit_myers in fused mode) rests on, checked against the CPU oracle on seeded
read/window pairs.  D = the unit-cost semi-global distance of the read to the window (first row 0, minimum of the last
row) under the SW matrix's match relation, where a read N matches a window N (ssw/src/lib.rs:11-16); the edit distance
of align.rs:28-85 is the same recurrence under the relation in which a read N matches nothing (index.rs:272-279).
  (a) read without N, or window without N  =>  D = the edit distance;
  (b) D <= ED    =>  SW score >= L - 2*ED  (index.rs:406 passes);
  (c) D > 2*ED   =>  SW score <  L - 2*ED  (index.rs:406 fails).
Lengths up to 253 bases: the range of the byte kernel, where the oracle's score is the exact local score."""
import math
import random

import numpy as np

import helpers
from oracle import oracle as O

EDIT_RATE = 0.13


def semi_global(read, win, n_matches_n):
    """min over the last row of the unit-cost matrix with an all-zero first row"""
    w = np.frombuffer(win, dtype=np.uint8)
    idx = np.arange(len(w) + 1)
    prev = np.zeros(len(w) + 1, dtype=np.int64)
    for i, r in enumerate(read, 1):
        eq = (w == r) if (n_matches_n or r != ord("N")) else np.zeros(len(w), dtype=bool)
        tmp = np.empty(len(w) + 1, dtype=np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(prev[:-1] + (~eq).astype(np.int64), prev[1:] + 1)
        prev = np.minimum.accumulate(tmp - idx) + idx  # the horizontal steps: D[i][j] <= D[i][j-1] + 1
    return int(prev.min())


def pairs(seed=20, per_length=100):
    rng = random.Random(seed)
    out = []
    for L in (40, 60, 100, 150, 253):
        ED = math.ceil(L * EDIT_RATE)
        for it in range(per_length):
            win = bytearray(helpers.rnd_seq(rng, L + 2 * ED))
            kind = it % 4  # 0: no N anywhere, 1: N runs in the window, 2: N in the read, 3: both (the read's N face the window's)
            if kind in (1, 3):
                for _ in range(rng.randrange(1, 4)):
                    k = rng.randrange(1, max(2, ED))
                    at = rng.randrange(0, len(win) - k)
                    win[at:at + k] = b"N" * k
            read = bytearray(win[ED:ED + L + 3 * ED])
            if kind == 1:
                read = bytearray(c if c != ord("N") else rng.choice(b"ACGT") for c in read)
            n_edits = rng.randrange(0, 3 * ED + 1) if it % 5 else rng.randrange(0, ED + 1)
            for _ in range(n_edits):
                at = rng.randrange(L)
                op = rng.randrange(4)
                if op <= 1:
                    read[at] = rng.choice(b"ACGT")
                elif op == 2:
                    del read[at]
                else:
                    read.insert(at, rng.choice(b"ACGT"))
            read = read[:L]
            if kind == 2:
                for at in rng.sample(range(L), rng.randrange(1, ED + 2)):
                    read[at] = ord("N")
            out.append((bytes(read), bytes(win), ED))
    return out


def test_one_distance_decides_prefilter_and_edit_distance():
    n_same = n_lower = n_pass = n_refuted = n_between = 0
    for read, win, ED in pairs():
        L = len(read)
        assert L <= 253
        d_sw = semi_global(read, win, True)
        d_edit = semi_global(read, win, False)
        assert d_edit == O.min_edit_distance(read.replace(b"N", b"."), win)
        assert d_sw <= d_edit
        if b"N" not in read or b"N" not in win:
            assert d_sw == d_edit, (read, win)  # (a)
            n_same += 1
        elif d_sw < d_edit:
            n_lower += 1
        score = O.ssw_score(read, win)
        if d_sw <= ED:
            assert score >= L - 2 * ED, (read, win, d_sw, score)  # (b)
            n_pass += 1
        elif d_sw > 2 * ED:
            assert score < L - 2 * ED, (read, win, d_sw, score)  # (c)
            n_refuted += 1
        else:
            n_between += 1
    # the inputs reach every case: the second pass is needed (D below the edit distance), both decided sides, the sweep's zone
    assert n_same >= 200 and n_lower >= 50 and n_pass >= 100 and n_refuted >= 30 and n_between >= 50, \
        (n_same, n_lower, n_pass, n_refuted, n_between)
