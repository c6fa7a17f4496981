"""The merge of per-chunk hit lists restated in Python from its description (no library code): shared by
test_chunk_merge_cpu.py and test_chunk_merge.py.

A database cut into chunks is binned chunk by chunk over the same reads.  The merged list holds, read by read in read
order, the hits of chunk 0, then of chunk 1, and so on; inside a chunk's share the hits keep the order the chunk's own
list has them in."""
import numpy as np


def merge_hits(parts):
    """parts: one structured hit array per chunk, each ordered by `read` -> the merged array"""
    parts = list(parts)
    if not parts:
        raise ValueError("no chunk")
    out = []
    cursor = [0] * len(parts)
    reads = sorted(set(int(r) for p in parts for r in p["read"]))
    for r in reads:
        for c, p in enumerate(parts):
            k = cursor[c]
            while k < len(p) and int(p["read"][k]) == r:
                out.append(p[k])
                k += 1
            cursor[c] = k
    assert cursor == [len(p) for p in parts], "a chunk's hits are not ordered by read"
    if not out:
        return np.zeros(0, dtype=parts[0].dtype)
    return np.array(out, dtype=parts[0].dtype)


def presence(hits, n):
    p = np.zeros(n, dtype=bool)
    p[hits["read"].astype(np.int64)] = True
    return p


def chunk_facts(parts, n):
    """what makes a chunked fixture worth its name: (reads with hits from two chunks or more, reads that carry a TaxID whose
    smallest edit differs between two chunks, per chunk the reads matched in that chunk only, reads without any hit)"""
    pres = np.stack([presence(p, n) for p in parts])
    several = int((pres.sum(axis=0) >= 2).sum())
    best = []
    for p in parts:
        d = {}
        for r, t, e in zip(p["read"].tolist(), p["tax_id"].tolist(), p["edit"].tolist()):
            d[r, t] = min(d.get((r, t), e), e)
        best.append(d)
    differ = set()
    for a in range(len(parts)):
        for b in range(a + 1, len(parts)):
            for key, e in best[a].items():
                if key in best[b] and best[b][key] != e:
                    differ.add(key[0])
    only = [int((pres[c] & (pres.sum(axis=0) == 1)).sum()) for c in range(len(parts))]
    return several, len(differ), only, int((pres.sum(axis=0) == 0).sum())
