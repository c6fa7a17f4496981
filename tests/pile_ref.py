"""The plain restatement of a pileup (include/mtsv_amd.h, "pileup"), shared by test_pile_cpu.py and test_pile.py.  Written
from the definition in the header: per hit place_ref's (start, end, ops), the ops walked base by base into a table
{(tax_id, gi): [[0] * 8 per slot]}, the best edit per read over the call's hits, the slack, the TaxID list, and the site
predicate in Python integers.  Nothing here comes from the device."""
import place_ref as R

SLACK_ALL = 0xffffffff
REF_NONE = 0xff
N_MATCH, N_DEL, N_INS = 0, 6, 7
HEADER = "taxid\tgi\tpos\tref\tdepth\tmatch\tA\tC\tG\tT\tN\tdel\tins\n"


def new_table(entries, taxa=None):
    """L + 1 zeroed slots for every reference of `entries` ((tax_id, gi, seq), ...) the TaxID list selects (None, empty: all)"""
    return {(t, g): [[0] * 8 for _ in range(len(s) + 1)] for t, g, s in entries if not taxa or t in taxa}


def ref_codes(seq):
    """the ref code of every slot: the text's code per position, REF_NONE for slot L"""
    return [int(c) for c in R.codes(seq)] + [REF_NONE]


def walk(slots, read, strand, start, ops):
    """one hit's ops into its reference's slots; returns (the slots it added to n[0..6], in order; read bases consumed)"""
    P = R.strand_codes(read, strand)
    i, j, touched = 0, start, []
    for n, op in ops:
        if op == R.OP_EQ:
            for k in range(n):
                slots[j + k][N_MATCH] += 1
                touched.append(j + k)
            i, j = i + n, j + n
        elif op == R.OP_X:
            for _ in range(n):
                slots[j][1 + int(P[i])] += 1
                touched.append(j)
                i, j = i + 1, j + 1
        elif op == R.OP_D:
            for _ in range(n):
                slots[j][N_DEL] += 1
                touched.append(j)
                j += 1
        else:
            assert op == R.OP_I
            slots[j][N_INS] += 1                      # once per run
            i += n
    return touched, i


def counted(hits, slack):
    """per hit of a call ((read, tax_id, gi, offset, edit, strand), ...): edit <= the read's smallest edit in the call + slack"""
    best = {}
    for h in hits:
        best[h[0]] = min(best.get(h[0], h[4]), h[4])
    return [slack == SLACK_ALL or h[4] <= min(best[h[0]] + slack, 0xffffffff) for h in hits]


def add_run(table, reads, hits, placed, slack):
    """one call: `placed` is place_ref's (start, end, ops) per hit; returns (hits piled, hits skipped)"""
    piled = skipped = 0
    for h, ok, pl in zip(hits, counted(hits, slack), placed):
        r, t, g, o, e, strand = h
        if (t, g) not in table:
            skipped += 1
        elif ok:
            walk(table[(t, g)], reads[r], strand, pl[0], pl[2])
            piled += 1
    return piled, skipped


def depth(n):
    return sum(n[:7])


def is_site(n, min_depth, min_alt, min_alt_ppm):
    d = depth(n)
    return d + n[N_INS] > 0 and d >= min_depth and any(n[c] >= min_alt and n[c] * 1000000 >= min_alt_ppm * d for c in range(1, 8))


def sites(table, seq_of, min_depth=0, min_alt=0, min_alt_ppm=0):
    """rows (tax_id, gi, pos, ref, [n0..n7]) ascending by (tax_id, gi, pos); seq_of: {(tax_id, gi): seq}"""
    rows = []
    for key in sorted(table):
        ref = ref_codes(seq_of[key])
        rows += [(key[0], key[1], pos, ref[pos], list(n)) for pos, n in enumerate(table[key]) if is_site(n, min_depth, min_alt, min_alt_ppm)]
    return rows


def line(tax_id, gi, pos, ref, n):
    letter = "ACGTN"[ref] if ref < 5 else "."
    return "\t".join(str(x) for x in (tax_id, gi, pos, letter, depth(n), *n)) + "\n"


def text(rows):
    """the text of mtsv_format_variants"""
    return HEADER + "".join(line(*r) for r in rows)
