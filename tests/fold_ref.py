"""The fold of two assignment lists restated in Python with dicts and tuples (no library code): shared by test_fold_cpu.py
and test_fold.py.

A list holds records of one grain, keys distinct.  The fold of two lists is their union in key order with one record per
key; where both lists hold a key the better value stays.

  grain      record                             key                           value kept for equal keys
  TAXID      (read, tax_id, edit)               (read, tax_id)                smallest edit
  LONG       (read, tax_id, gi, offset, edit)   (read, tax_id, gi, offset)    smallest edit
  TAXID_GI   (read, tax_id, gi, offset, edit)   (read, tax_id, gi)            smallest (edit, offset)

Every field is a non-negative Python int, so tuples compare as the unsigned fields do.  report() and flags() derive what is
counted per read from a record list alone: per read {tax_id -> smallest edit of its records}, classified as
taxa_report_ref.classify does, and one flag per read that has a record."""
import numpy as np

import taxa_report_ref as R

TAXID, TAXID_GI, LONG = 0, 1, 2  # MTSV_GRAIN_*


def split(grain, rec):
    """(key, value) of a record"""
    if grain == TAXID:
        r, t, e = rec
        return (r, t), (e,)
    r, t, g, o, e = rec
    if grain == LONG:
        return (r, t, g, o), (e,)
    if grain == TAXID_GI:
        return (r, t, g), (e, o)
    raise ValueError(grain)


def join(grain, key, val):
    if grain == TAXID:
        return (*key, val[0])
    if grain == LONG:
        return (*key, val[0])
    return (*key, val[1], val[0])


def fold(grain, a, b):
    """the fold of lists a and b (either may be in any order; the result is in key order)"""
    d = {}
    for rec in list(a) + list(b):
        k, v = split(grain, rec)
        if k not in d or v < d[k]:
            d[k] = v
    return [join(grain, k, d[k]) for k in sorted(d)]


def fold_all(grain, lists):
    acc = []
    for l in lists:
        acc = fold(grain, acc, l)
    return acc


def is_list(grain, recs):
    """keys strictly ascending: what a list must be"""
    keys = [split(grain, r)[0] for r in recs]
    return all(a < b for a, b in zip(keys, keys[1:]))


def report(recs):
    """({tax_id: [only_hit, only_best, tied_best, not_best]}, reads with a record)"""
    return R.classify([r[0] for r in recs], [r[1] for r in recs], [r[-1] for r in recs])


def flags(recs, n):
    p = np.zeros(n, dtype=bool)
    for r in recs:
        p[r[0]] = True
    return p
