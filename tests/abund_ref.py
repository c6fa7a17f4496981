"""The definition of mtsv_fold_abundance (include/mtsv_amd.h) restated in plain Python: a dict per read, Python's int for every
mass, sum and weight, and float only for the one IEEE division of a share.  The weights of mtsv_abundance_weights and the TSV of
mtsv_format_abundance are here too.  Nothing of the library is used."""
import math

ALL = 0xffffffff
ONE = 1 << 32
HEADER = "taxid\tmass\tabundance_pct\treads_any\treads_unique\tassigned\n"


def weights(q, n_w):
    """w[d - 1] = min(floor(q^d * 2^32), 2^32 - 1), the power by repeated multiplication in double precision"""
    if not (0.0 < q <= 1.0) or not 1 <= n_w <= 255:
        raise ValueError("q in (0, 1], n_w in 1 .. 255")
    w, x = [], 1.0
    for _ in range(n_w):
        x = x * q
        w.append(min(int(math.floor(x * 4294967296.0)), ONE - 1))
    return w


def entries(recs, slack):
    """recs: (read, tax, edit) or wide (read, tax, gi, offset, edit) records -> {read: {tax: (d, e)}} of the entering taxa, reads
    and taxa in ascending order"""
    e = {}
    for r in recs:
        read, tax, edit = r[0], r[1], r[-1]
        per = e.setdefault(read, {})
        per[tax] = min(per.get(tax, edit), edit)
    out = {}
    for read in sorted(e):
        m = min(e[read].values())
        out[read] = {t: (e[read][t] - m, e[read][t]) for t in sorted(e[read]) if e[read][t] - m <= slack}
    return out


def weight_of(d, w):
    return ONE if d == 0 else w[min(d, len(w)) - 1]


def shares(per, A, w):
    """steps 1 to 4 for one read: ({tax: x}, {tax: q})"""
    x = {t: (A[t] * weight_of(d, w)) >> 48 for t, (d, _) in per.items()}
    s = sum(x.values())
    if s == 0:
        x = {t: weight_of(d, w) >> 17 for t, (d, _) in per.items()}
        s = sum(x.values())
    return x, {t: int((float(x[t]) / float(s)) * 4294967296.0) for t in per}


def run(recs, w, slack=ALL, max_iters=100, tol=0, start=ONE):
    """-> dict(rows=[(tax, mass, reads_any, reads_unique, assigned)], info={...}, assigned=[(read, tax, edit)], history=[(A, L1)])"""
    ent = entries(recs, slack)
    taxa = sorted({t for per in ent.values() for t in per})
    if len(ent) >= 1 << 31 or any(len(per) >= 65536 for per in ent.values()):
        raise OverflowError("limit")
    A = {t: start for t in taxa}
    iterations, converged, l1, history = 0, 0, 0, []
    while iterations < max_iters:
        nxt = {t: 0 for t in taxa}
        for per in ent.values():
            for t, q in shares(per, A, w)[1].items():
                nxt[t] += q
        l1 = sum(abs(nxt[t] - A[t]) for t in taxa)
        A = nxt
        iterations += 1
        history.append((dict(A), l1))
        if l1 <= tol:
            converged = 1
            break
    assigned = []
    for read, per in ent.items():
        x = shares(per, A, w)[0]
        best = min(per, key=lambda t: (-x[t], t))
        assigned.append((read, best, per[best][1]))
    n_any, n_unique, n_assigned = ({t: 0 for t in taxa} for _ in range(3))
    for per in ent.values():
        for t in per:
            n_any[t] += 1
            n_unique[t] += len(per) == 1
    for _, t, _ in assigned:
        n_assigned[t] += 1
    rows = [(t, A[t], n_any[t], n_unique[t], n_assigned[t]) for t in taxa]
    info = dict(reads=len(ent), entries=sum(len(per) for per in ent.values()), taxa=len(taxa), total_mass=sum(A.values()),
                l1_change=l1 if iterations else 0, iterations=iterations, converged=converged)
    return dict(rows=rows, info=info, assigned=assigned, history=history)


def tsv(rows, total_mass):
    total = max(total_mass, 1)
    text = HEADER
    for t, mass, any_, unique, assigned in rows:
        text += "%d\t%.6f\t%.4f\t%d\t%d\t%d\n" % (t, float(mass) / 4294967296.0, float(mass) * 100.0 / float(total), any_, unique, assigned)
    return text.encode()


def lines(assigned, ids):
    """the result lines of the assigned records, READ_ID:TAXID=EDIT"""
    return "".join(f"{ids[r]}:{t}={e}\n" for r, t, e in assigned).encode()


# the worked example of the header
EXAMPLE = [(0, 5, 0), (1, 5, 1), (1, 7, 1), (2, 5, 2), (2, 7, 0), (3, 9, 3)]
EXAMPLE_AFTER = [({5: 7301444403, 7: 5583457484, 9: 4294967296}, 4294967295),
                 ({5: 7786955038, 7: 5097946848, 9: 4294967296}, 971021271),
                 ({5: 8077478865, 7: 4807423021, 9: 4294967296}, 581047654)]
EXAMPLE_ASSIGNED = [(0, 5, 0), (1, 5, 1), (2, 7, 0), (3, 9, 3)]
EXAMPLE_ROWS_COUNTS = {5: (3, 1, 2), 7: (2, 0, 1), 9: (1, 1, 1)}
EXAMPLE_TOTAL_MASS = 17179869182
