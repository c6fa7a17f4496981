"""The plain-Python restatement of mtsv_coverage (include/mtsv_amd.h), shared by test_coverage_cpu.py and test_coverage.py.
Written from the description in the header, not from the kernels: a dict from (tax_id, gi) to [length, set of reads,
alignments, aligned_bases, bytearray of positions], and a loop over the records."""
import collections

SLACK_ALL = 0xffffffff
LENGTH, READS, ALIGNMENTS, BASES, POSITIONS = range(5)
HEADER = "taxid\tgi\tlength\treads\talignments\taligned_bases\tdepth\tcovered_bases\tbreadth_pct\n"


class Refused(Exception):
    """what the library answers with MTSV_E_ARG: nothing has been added"""


class Coverage:
    def __init__(self, refs=()):
        self.table = {}
        self.calls = 0
        self.add_refs(refs)

    def add_refs(self, refs):
        """refs: (tax_id, gi, length); the same (tax_id, gi) twice is one reference with the larger length"""
        for t, g, length in refs:
            have = self.table.get((t, g))
            if have is None:
                self.table[(t, g)] = [length, set(), 0, 0, bytearray(length)]
            elif length > have[LENGTH]:
                have[LENGTH] = length
                have[POSITIONS].extend(bytes(length - len(have[POSITIONS])))

    def reset(self):
        for row in self.table.values():
            row[READS], row[ALIGNMENTS], row[BASES], row[POSITIONS] = set(), 0, 0, bytearray(row[LENGTH])

    def add_fold(self, recs, read_len, slack=0):
        """recs: (read, tax_id, gi, offset, edit) of one fold; read_len: by read"""
        for r, t, g, o, e in recs:
            if (t, g) not in self.table:
                raise Refused(f"reference ({t}, {g}) is not in the table")
            if o >= self.table[(t, g)][LENGTH]:
                raise Refused(f"offset {o} at or beyond the end of reference ({t}, {g})")
        best = {}
        for r, t, g, o, e in recs:
            best[r] = min(best.get(r, e), e)
        for r, t, g, o, e in recs:
            if e > min(best[r] + slack, SLACK_ALL):
                continue
            row = self.table[(t, g)]
            end = min(o + read_len[r], row[LENGTH])
            row[READS].add((self.calls, r))             # the reads of different calls are different reads
            row[ALIGNMENTS] += 1
            row[BASES] += end - o
            row[POSITIONS][o:end] = b"\1" * (end - o)
        self.calls += 1

    def rows(self):
        """every reference, ascending by (tax_id, gi): (tax_id, gi, length, reads, alignments, aligned_bases, covered_bases)"""
        return [(t, g, row[LENGTH], len(row[READS]), row[ALIGNMENTS], row[BASES], sum(row[POSITIONS]))
                for (t, g), row in sorted(self.table.items())]


def rows_of(refs, folds, slack=0):
    """the rows after the folds [(recs, read_len), ..] have been added to a table of refs"""
    c = Coverage(refs)
    for recs, read_len in folds:
        c.add_fold(recs, read_len, slack)
    return c.rows()


def _line(t, g, length, reads, alignments, bases, covered):
    depth = bases / length if length else 0.0
    breadth = covered / length * 100.0 if length else 0.0
    return f"{t}\t{g}\t{length}\t{reads}\t{alignments}\t{bases}\t{depth:.2f}\t{covered}\t{breadth:.2f}\n"


def report(rows):
    """the text of mtsv_format_coverage_report"""
    by_taxon = collections.OrderedDict()
    for row in rows:
        by_taxon.setdefault(row[0], []).append(row)
    text = HEADER
    for t, group in by_taxon.items():
        hit = [row for row in group if row[4] > 0]
        for row in hit:
            text += _line(*row)
        if hit:
            text += _line(t, "*", *[sum(row[k] for row in group) for k in range(2, 7)])
    return text.encode()


def as_tuples(a):
    """a REF_COVERAGE_DTYPE array as the tuples of rows()"""
    return [tuple(int(x) for x in row) for row in a.tolist()]
