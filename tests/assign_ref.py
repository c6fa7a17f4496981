"""The assignments of a batch, restated in Python: what mtsv-binner writes per read in its default format
(write_assignments, binner.rs:355-378) and what mtsv-collapse --mode taxid makes of several result files
(collapse.rs:269-297).  Per read a dict tax_id -> smallest edit over all of the read's hits (both strands, every
chunk), emitted ascending by tax_id.  The tests feed it the CPU oracle's hits, never the device's."""
import numpy as np


def collapse(hits):
    """hits: any array with read, tax_id and edit fields, in any order.  Returns the (read, tax_id, edit) records as a list
    of int triples: reads ascending, inside a read tax_id ascending, edit the smallest of the pair's hits."""
    per_read = {}
    for r, t, e in zip(hits["read"].tolist(), hits["tax_id"].tolist(), hits["edit"].tolist()):
        d = per_read.setdefault(r, {})
        if t not in d or e < d[t]:
            d[t] = e
    return [(r, t, per_read[r][t]) for r in sorted(per_read) for t in sorted(per_read[r])]


def as_triples(a):
    """a downloaded ASSIGN_DTYPE array as the list collapse() returns"""
    return list(zip(a["read"].tolist(), a["tax_id"].tolist(), a["edit"].tolist()))


def as_array(triples, dtype):
    out = np.zeros(len(triples), dtype=dtype)
    for i, (r, t, e) in enumerate(triples):
        out[i] = (r, t, e)
    return out


def text(triples, read_ids):
    """READ_ID:TAXID=EDIT,... -- one line per read that has a record, in read order"""
    lines, cur, items = [], None, []
    for r, t, e in triples:
        if r != cur:
            if cur is not None:
                lines.append(f"{read_ids[cur]}:{','.join(items)}\n")
            cur, items = r, []
        items.append(f"{t}={e}")
    if cur is not None:
        lines.append(f"{read_ids[cur]}:{','.join(items)}\n")
    return "".join(lines)
