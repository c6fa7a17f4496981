"""The plain restatement of the consensus of a pileup (include/mtsv_amd.h, "consensus"), shared by test_consensus_cpu.py and
test_consensus.py.  Written from the definition in the header, over pile_ref's table {(tax_id, gi): [[n0 .. n7] per slot]}: a
loop per position, Python integers only.  It produces the rows, the FASTA text and the statistics' text.  Nothing here comes
from the device."""
import pile_ref as PR
import place_ref as R

FILL_N, FILL_REF = 0, 1
FIELDS = ("tax_id", "gi", "length", "covered", "n_ref", "n_sub", "n_del", "n_low", "n_ambig", "ins_sites", "sum_depth")
HEADER = "taxid\tgi\tlength\tcovered\tbreadth_pct\tmean_depth\tcons_len\tref\tsub\tdel\tlow\tambiguous\tins_sites\tidentity_pct\n"
LOW, AMBIG, REF, SUB, DEL = "low", "ambig", "ref", "sub", "del"


def classify(n, md, min_frac_ppm):
    """(class, w) of a position's counters"""
    depth = sum(n[:7])
    if depth < md:
        return LOW, None
    w = 0
    for c in range(1, 7):
        if n[c] > n[w]:                                   # the lowest channel wins a tie
            w = c
    if w == 5 or n[w] * 1000000 < min_frac_ppm * depth:
        return AMBIG, w
    return (REF if w == 0 else DEL if w == 6 else SUB), w


def call_reference(slots, seq, min_depth, min_frac_ppm, fill):
    """(the consensus characters as a str, the row's counters as a dict) of one reference: slots [L + 1][8], seq its L bases"""
    md = max(min_depth, 1)
    L = len(seq)
    assert len(slots) == L + 1
    codes = [int(c) for c in R.codes(seq)]
    row = dict(length=L, covered=0, n_ref=0, n_sub=0, n_del=0, n_low=0, n_ambig=0, ins_sites=0, sum_depth=0)
    out = []
    for p in range(L):
        n = slots[p]
        depth = sum(n[:7])
        row["sum_depth"] += depth
        if depth >= md:
            row["covered"] += 1
        kind, w = classify(n, md, min_frac_ppm)
        filler = "N" if fill == FILL_N else "acgtn"[codes[p]]
        if kind == LOW:
            row["n_low"] += 1
            out.append(filler)
        elif kind == AMBIG:
            row["n_ambig"] += 1
            out.append(filler)
        elif kind == REF:
            row["n_ref"] += 1
            out.append("ACGTN"[codes[p]])
        elif kind == SUB:
            row["n_sub"] += 1
            out.append("ACGT"[w - 1])
        else:
            row["n_del"] += 1
    for j in range(L + 1):
        D = sum(slots[j][:7]) if j < L else 0
        if slots[j][7] >= md and 2 * slots[j][7] > D:
            row["ins_sites"] += 1
    return "".join(out), row


def wrap(chars, line_width):
    if not chars:
        return ""
    if line_width == 0:
        return chars + "\n"
    return "".join(chars[k:k + line_width] + "\n" for k in range(0, len(chars), line_width))


def consensus(table, seq_of, min_depth=1, min_frac_ppm=500000, min_breadth_ppm=0, fill=FILL_N, line_width=60):
    """(the FASTA text, the emitted references' rows as tuples in the order of FIELDS), ascending by (tax_id, gi)"""
    text, rows = [], []
    for key in sorted(table):
        chars, row = call_reference(table[key], seq_of[key], min_depth, min_frac_ppm, fill)
        assert row["length"] == row["covered"] + row["n_low"] and row["covered"] == row["n_ref"] + row["n_sub"] + row["n_del"] + row["n_ambig"]
        assert len(chars) == row["length"] - row["n_del"]
        if not (row["covered"] >= 1 and row["covered"] * 1000000 >= min_breadth_ppm * row["length"]):
            continue
        rows.append((key[0], key[1]) + tuple(row[f] for f in FIELDS[2:]))
        text.append(">%d-%d\n" % (key[1], key[0]) + wrap(chars, line_width))
    return "".join(text), rows


def ratio(a, b, scale=1.0):
    return "%.2f" % (a / b * scale if b else 0.0)


def stats_line(tax_id, gi, length, covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites, sum_depth):
    return "\t".join(str(x) for x in (tax_id, gi, length, covered, ratio(covered, length, 100.0), ratio(sum_depth, length), length - n_del, n_ref, n_sub,
                                      n_del, n_low, n_ambig, ins_sites, ratio(n_ref, n_ref + n_sub + n_del, 100.0))) + "\n"


def stats_text(rows):
    """the text of mtsv_format_consensus_stats: after a TaxID's rows one line with gi `*` of their sums"""
    out, k = [HEADER], 0
    while k < len(rows):
        j = k
        while j < len(rows) and rows[j][0] == rows[k][0]:
            out.append(stats_line(*rows[j]))
            j += 1
        out.append(stats_line(rows[k][0], "*", *(sum(r[f] for r in rows[k:j]) for f in range(2, 11))))
        k = j
    return "".join(out)
