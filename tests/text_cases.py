"""Synthetic record lists and read-ID tables for the result lines written on the device (k_text.hip, mtsv_fold_format_text,
mtsv_batch_format_text): shared by test_text_cpu.py and test_text.py.

A case is a Case(records, ids, table, second): `records` a list of one grain in key order (tuples as assign_ref / grain_ref
use them), `ids` the reads' IDs as str (what strnlen finds in a slot), `table` the same IDs as the (bytes, offsets) pair the
C ABI takes -- a slot is the ID and one NUL, the ID and several NULs, or the ID alone with no NUL -- and `second` another list
of the grain to fold into the first.  The expected text never comes from the library: expected() applies the restatements
assign_ref.text / grain_ref.text, which the existing suites pin against the host formatters."""
import collections
import ctypes as C
import random

import numpy as np

import assign_ref as A
import fold_ref as F
import grain_ref as GR
from mtsv_tools_amd import _lib

Case = collections.namedtuple("Case", "records ids table second")

GRAINS = {"taxid": F.TAXID, "long": F.LONG, "taxid_gi": F.TAXID_GI}
TILE = 64
# every power of ten from both sides, the largest value, and two more with bit 31 set
LADDER = sorted({0, 4294967295, 2147483648, 3000000000} | {10 ** k for k in range(1, 10)} | {10 ** k - 1 for k in range(1, 10)})
ID_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 5000)
ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_/.|"


def text(grain, records, ids):
    return (A.text(records, ids) if grain == F.TAXID else GR.text(records, ids)).encode()


def expected(grain, case):
    return text(grain, case.records, case.ids)


def rec(grain, read, tax, gi, offset, edit):
    return (read, tax, edit) if grain == F.TAXID else (read, tax, gi, offset, edit)


def make_id(rng, read, length):
    """an ID of exactly `length` bytes that names its read where there is room"""
    head = f"r{read}|"
    return (head + "".join(rng.choice(ALPHABET) for _ in range(length)))[:length]


def make_table(rng, ids):
    """the IDs as slots of the three kinds in turn (from a random start)"""
    blob, off = bytearray(), [0]
    for i, s in enumerate(ids):
        kind = (i + rng.randrange(3)) % 3
        blob += s.encode() + (b"\0", b"\0" * rng.randrange(2, 6), b"")[kind]
        off.append(len(blob))
    return bytes(blob), np.array(off, dtype=np.uint64)


def second_list(grain, rng, records, n_reads):
    """every third record with a smaller (or equal) edit, and a record of a read that had none, where there is one"""
    out = [(*r[:-1], r[-1] // 2) for r in records[::3]]
    free = sorted(set(range(n_reads)) - {r[0] for r in records})
    if free:
        out.append(rec(grain, rng.choice(free), 77, 8, 9, 3))
    return sorted(out)


def finish(grain, rng, records, lengths):
    """lengths: the ID length of every read, with or without records; the reads without get an ID that says so"""
    have = {r[0] for r in records}
    ids = [make_id(rng, i, n) if i in have else f"ABSENT{i}|" + "x" * n for i, n in enumerate(lengths)]
    return Case(records, ids, make_table(rng, ids), second_list(grain, rng, records, len(ids)))


def spread(grain, rng, n, max_id=20):
    """n records over reads of one to three records each, with gaps in the read numbers"""
    records, read = [], 0
    while len(records) < n:
        read += rng.randrange(1, 4)
        for k in range(min(rng.randrange(1, 4), n - len(records))):
            records.append(rec(grain, read, 10 * k + rng.randrange(10), rng.randrange(1000), rng.randrange(100000), rng.randrange(12)))
    return finish(grain, rng, records, [rng.randrange(max_id + 1) for _ in range(read + 2)])


def run_of(grain, read, n, first=0):
    """n records of one read, keys ascending in every grain"""
    if grain == F.TAXID:
        return [(read, first + k, (7 * k) % 13) for k in range(n)]
    return [(read, first + k // 4, k % 4, 0, (7 * k) % 13) for k in range(n)]


def cases(grain):
    rng = random.Random(500 + grain)
    L = len(LADDER)
    out = {}
    # every field through every power of ten, in reads whose IDs have every length; reads in between have no records
    with_records = (1, 2, 4, 7, 8, 11, 12, 13, 17, 19)
    records = []
    for j, read in enumerate(with_records):
        records += [rec(grain, read, LADDER[k], LADDER[(k + 3 + j) % L], LADDER[(k + 7 + 2 * j) % L], LADDER[(k + 11 + 3 * j) % L]) for k in range(L)]
    lengths = [9] * 23
    for j, read in enumerate(with_records):
        lengths[read] = ID_LENGTHS[j]
    out["ladder"] = finish(grain, rng, records, lengths)
    if grain != F.TAXID:  # keys that differ in the later fields only
        same_tax = [rec(grain, 3, 5, LADDER[k], LADDER[L - 1 - k], k) for k in range(L)]
        if grain == F.LONG:
            same_tax += [rec(grain, 5, 5, 6, LADDER[k], LADDER[k]) for k in range(L)]
        out["later_fields"] = finish(grain, rng, same_tax, [7] * 9)
    for n in (0, 1, 63, 64, 65, 197):
        out[f"size_{n}"] = spread(grain, rng, n)
    out["head_at_64"] = finish(grain, rng, run_of(grain, 2, 64) + run_of(grain, 5, 9), [12] * 8)
    out["straddle_63_64"] = finish(grain, rng, run_of(grain, 0, 60) + run_of(grain, 3, 11) + run_of(grain, 4, 2), [6, 0, 0, 5, 64, 65])
    out["one_read_of_six_tiles"] = finish(grain, rng, run_of(grain, 1, 5 * TILE + 70), [3, 31, 3])
    out["single_record_reads"] = spread(grain, rng, 40 * TILE + 5, max_id=13)
    # more text than one LDS window holds at the default tile, most IDs copied by the workgroup
    many = [rec(grain, 2 * i + 1, i % 50, i % 7, i, i % 10) for i in range(1100)]
    out["many_long_ids"] = finish(grain, rng, many, [(3, 255, 65, 70)[i % 4] for i in range(2 * 1100 + 1)])
    return out


def tile_edges(grain, case, tile=TILE):
    """the byte at which every tile of `tile` records begins, and the end of the text"""
    n = len(case.records)
    return [len(text(grain, case.records[:k], case.ids)) for k in range(0, n, tile)] + [len(expected(grain, case))]


def host_format(grain, records, table):
    """mtsv_format_assignments / _gi on a raw ID table (host only)"""
    blob, off = table
    a = A.as_array(records, _lib.ASSIGN_DTYPE) if grain == F.TAXID else GR.as_array(records, _lib.ASSIGN_GI_DTYPE)
    call = _lib.lib().mtsv_format_assignments if grain == F.TAXID else _lib.lib().mtsv_format_assignments_gi
    out, n = C.c_void_p(), C.c_uint64()
    _lib._check(call(a.ctypes.data, len(a), blob, off.ctypes.data, len(off) - 1, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        _lib.lib().mtsv_free(out)
