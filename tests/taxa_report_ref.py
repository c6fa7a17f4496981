"""The taxa report's semantics restated in Python from their description (no reference code): shared by
test_taxa_report_cpu.py and test_taxa_report.py.

Per read with at least one hit: summary = {tax_id -> smallest edit over the read's hits}; total_reads += 1.  With m the
smallest edit of the summary and best the number of its entries at m, each TaxID t of the summary adds one to exactly
one of its counters: only_hit if the summary has one entry, else only_best if summary[t] == m and best == 1, else
tied_best if summary[t] == m, else not_best.  Reads without hits count nowhere."""
import numpy as np

COLS = ("only_hit", "only_best", "tied_best", "not_best")
HEADER = "taxid\tonly_hit\tonly_hit_pct\tonly_best\tonly_best_pct\ttied_best\ttied_best_pct\tnot_best\tnot_best_pct\ttotal_reads\ttotal_pct\n"


def classify(read, tax_id, edit):
    """hit arrays (read, tax_id, edit), in any order -> ({tax_id: [only_hit, only_best, tied_best, not_best]}, total_reads)"""
    per_read = {}
    for r, t, e in zip(np.asarray(read).tolist(), np.asarray(tax_id).tolist(), np.asarray(edit).tolist()):
        s = per_read.setdefault(r, {})
        s[t] = min(s.get(t, e), e)
    stats = {}
    for s in per_read.values():
        m = min(s.values())
        best = sum(1 for e in s.values() if e == m)
        for t, e in s.items():
            row = stats.setdefault(t, [0, 0, 0, 0])
            if len(s) == 1:
                row[0] += 1
            elif e == m and best == 1:
                row[1] += 1
            elif e == m:
                row[2] += 1
            else:
                row[3] += 1
    return stats, len(per_read)


def classify_hits(hits):
    return classify(hits["read"], hits["tax_id"], hits["edit"])


def rows_array(stats, dtype):
    """the dict of classify() as the structured array the library returns: ascending tax_id"""
    out = np.zeros(len(stats), dtype=dtype)
    for i, t in enumerate(sorted(stats)):
        out[i] = (t, *stats[t])
    return out


def rows_dict(rows):
    return {int(r["tax_id"]): [int(r[c]) for c in COLS] for r in rows}


def parse_results(text):
    """default-format result lines `id:tax=edit,...` -> hit arrays with one read number per line"""
    read, tax, edit = [], [], []
    ids = []
    for k, line in enumerate(text.splitlines()):
        rid, rest = line.rsplit(":", 1)
        ids.append(rid)
        for tok in rest.split(","):
            t, e = tok.split("=")
            read.append(k)
            tax.append(int(t))
            edit.append(int(e))
    return ids, np.array(read, np.uint64), np.array(tax, np.uint32), np.array(edit, np.uint32)


def parse_report(text):
    """a report TSV -> (rows dict, the text's lines)"""
    lines = text.splitlines()
    assert lines[0] + "\n" == HEADER
    rows = {}
    for line in lines[1:]:
        f = line.split("\t")
        assert len(f) == 11
        rows[int(f[0])] = [int(f[1]), int(f[3]), int(f[5]), int(f[7])]
        assert int(f[9]) == sum(rows[int(f[0])])
    return rows
