"""The wide assignments of a batch, restated in Python.  collapse_long: what mtsv-binner --output-format long writes per
read (binner.rs:320-352) -- per (tax_id, gi, offset) the smallest edit, ascending by the triple.  collapse_taxid_gi: what
mtsv-collapse --mode taxid-gi makes of long files (collapse.rs:603-625) -- per (tax_id, gi) the lexicographically smallest
(edit, offset), ascending by the pair.  Both over all of a read's hits (both strands, every chunk); every field compares as
an unsigned integer.  The tests feed them the CPU oracle's hits, never the device's."""
import numpy as np


def _fields(hits):
    return zip(hits["read"].tolist(), hits["tax_id"].tolist(), hits["gi"].tolist(), hits["offset"].tolist(), hits["edit"].tolist())


def collapse_long(hits):
    """(read, tax_id, gi, offset, edit) tuples: reads ascending, inside a read (tax_id, gi, offset) ascending"""
    per_read = {}
    for r, t, g, o, e in _fields(hits):
        d = per_read.setdefault(r, {})
        k = (t, g, o)
        if k not in d or e < d[k]:
            d[k] = e
    return [(r, t, g, o, per_read[r][(t, g, o)]) for r in sorted(per_read) for t, g, o in sorted(per_read[r])]


def collapse_taxid_gi(hits):
    """(read, tax_id, gi, offset, edit) tuples: reads ascending, inside a read (tax_id, gi) ascending; (edit, offset) the
    smallest of the pair's hits"""
    per_read = {}
    for r, t, g, o, e in _fields(hits):
        d = per_read.setdefault(r, {})
        k = (t, g)
        if k not in d or (e, o) < d[k]:
            d[k] = (e, o)
    return [(r, t, g, per_read[r][(t, g)][1], per_read[r][(t, g)][0]) for r in sorted(per_read) for t, g in sorted(per_read[r])]


def as_tuples(a):
    """a downloaded ASSIGN_GI_DTYPE array as the lists above"""
    return list(zip(a["read"].tolist(), a["tax_id"].tolist(), a["gi"].tolist(), a["offset"].tolist(), a["edit"].tolist()))


def as_array(records, dtype):
    out = np.zeros(len(records), dtype=dtype)
    for i, (r, t, g, o, e) in enumerate(records):
        out[i] = (r, t, g, o, e)
    return out


def text(records, read_ids):
    """READ_ID:TAXID-GI-OFFSET=EDIT,... -- one line per read that has a record, in read order"""
    lines, cur, items = [], None, []
    for r, t, g, o, e in records:
        if r != cur:
            if cur is not None:
                lines.append(f"{read_ids[cur]}:{','.join(items)}\n")
            cur, items = r, []
        items.append(f"{t}-{g}-{o}={e}")
    if cur is not None:
        lines.append(f"{read_ids[cur]}:{','.join(items)}\n")
    return "".join(lines)
