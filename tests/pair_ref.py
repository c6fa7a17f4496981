"""mtsv_fold_pair restated in Python with a dict per pair and a double loop (no library code): shared by test_pair_cpu.py and
test_pair.py.  Written from the description in include/mtsv_amd.h, not from the kernels.

Records are tuples whose first field is the read, second the TaxID and last the edit: (read, tax_id, edit) at the TAXID grain,
(read, tax_id, gi, offset, edit) at the two wide ones.  Reads 2p and 2p + 1 are the mates of pair p.  Every field is a
non-negative Python int, so the comparisons are the unsigned ones and nothing wraps."""
BOTH, EITHER, PROPER = 0, 1, 2  # MTSV_PAIR_*
U32 = 2 ** 32 - 1


def by_pair(records):
    """{pair: ([records of mate 0], [records of mate 1])}"""
    pairs = {}
    for r in records:
        pairs.setdefault(r[0] >> 1, ([], []))[r[0] & 1].append(r)
    return pairs


def smallest(recs):
    """{tax_id: the smallest edit among recs}"""
    m = {}
    for r in recs:
        m[r[1]] = min(m.get(r[1], r[-1]), r[-1])
    return m


def join_pair(mode, mate0, mate1, max_insert=0, unpaired_edits=0):
    """{tax_id: edit} of one pair"""
    m0, m1 = smallest(mate0), smallest(mate1)
    if mode == BOTH:
        return {t: m0[t] + m1[t] for t in m0 if t in m1}
    if mode == EITHER:
        out = {}
        for t in set(m0) | set(m1):
            if t in m0 and t in m1:
                out[t] = m0[t] + m1[t]
            else:
                out[t] = (m0[t] if t in m0 else m1[t]) + unpaired_edits
        return out
    if mode != PROPER:
        raise ValueError(mode)
    out = {}
    for a in mate0:
        for b in mate1:
            if a[1:3] == b[1:3] and abs(a[3] - b[3]) <= max_insert:
                e = a[-1] + b[-1]
                out[a[1]] = min(out.get(a[1], e), e)
    return out


def pair(mode, records, max_insert=0, unpaired_edits=0):
    """[(pair, tax_id, edit)] in key order"""
    out = []
    for p, (mate0, mate1) in by_pair(records).items():
        out += [(p, t, e) for t, e in join_pair(mode, mate0, mate1, max_insert, unpaired_edits).items()]
    return sorted(out)


def stats(records, n_reads, joined):
    """mtsv_pair_stats as a dict, from the records of f and the list pair() gave"""
    pairs = by_pair(records)
    return {"pairs": n_reads // 2,
            "both_mates_hit": sum(1 for a, b in pairs.values() if a and b),
            "one_mate_hit": sum(1 for a, b in pairs.values() if bool(a) != bool(b)),
            "joined": len({r[0] for r in joined}),
            "records": len(joined)}


def stem(id0, id1):
    """the ID of a pair from its mates' IDs: the common ID, or the common stem of `x/1` and `x/2`; None when they do not agree"""
    if id0 == id1:
        return id0
    if id0.endswith("/1") and id1.endswith("/2") and id0[:-2] == id1[:-2]:
        return id0[:-2]
    return None


def lines(joined, pair_ids):
    """the results text: PAIR_ID:TAXID=EDIT,... per pair with a record"""
    out, at = [], 0
    while at < len(joined):
        end = at
        while end < len(joined) and joined[end][0] == joined[at][0]:
            end += 1
        out.append(pair_ids[joined[at][0]] + ":" + ",".join(f"{t}={e}" for _, t, e in joined[at:end]) + "\n")
        at = end
    return "".join(out).encode()
