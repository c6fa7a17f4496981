"""Taxonomy, per-read LCA and clade report restated in Python (no library code): shared by test_lca_cpu.py and test_lca.py.
Written from the description of mtsv_taxonomy and mtsv_fold_lca in include/mtsv_amd.h, not from the kernels: the LCA here is
the deepest common member of the ancestor chains (lca), deliberately not the preorder-interval form the device uses -- that
form is restated apart (lca_by_intervals) and the two are compared on random sets.

A taxonomy is parsed from the text of a nodes.dmp.  parent[t] is the parent's TaxID, 0 for roots and implied roots; the
super-root is TaxID 0; a TaxID the file does not know is a child of the super-root.  Records are tuples whose first field is
the read, second the TaxID and last the edit (any grain)."""

U32 = 2 ** 32 - 1
UNKNOWN = "-"
HEADER = "taxid\tparent\trank\tdepth\tdirect\tdirect_pct\tclade\tclade_pct\n"


class Format(Exception):
    def __init__(self, line, what):
        super().__init__(f"line {line}: {what}")
        self.line = line


def number(s):
    if not 1 <= len(s) <= 10 or any(c not in "0123456789" for c in s):
        return None
    v = int(s)
    return v if v <= U32 else None


class Taxonomy:
    def __init__(self, text):
        self.parent, self.rank, listed_on = {}, {}, {}
        self._chains = None  # (chain() remembers its answers once the tree stands)
        raw = {}
        for no, line in enumerate(text.split("\n"), 1):
            if not line.strip(" \t\r"):
                continue
            fields = [f.strip(" \t\r") for f in line.split("|")]
            if len(fields) < 3:
                raise Format(no, "fewer than three fields")
            t, p = number(fields[0]), number(fields[1])
            if t is None or p is None:
                raise Format(no, "an ID that is not 1 to 10 digits up to 4294967295")
            if t == 0 or p == 0:
                raise Format(no, "TaxID 0")
            raw.setdefault(t, []).append((no, p, fields[2]))
        # (the library sorts by TaxID first: of several TaxIDs listed twice it names the smallest, at its second line)
        for t in sorted(raw):
            if len(raw[t]) > 1:
                raise Format(raw[t][1][0], f"TaxID {t} listed twice")
        for t, ((no, p, rank),) in raw.items():
            self.parent[t] = 0 if p == t else p
            self.rank[t] = rank
            listed_on[t] = no
        self.listed = sorted(self.parent)
        self.implied = sorted({p for p in self.parent.values() if p and p not in self.parent})
        for p in self.implied:
            self.parent[p] = 0
        self.rank_names = sorted({r.encode() for r in self.rank.values()})
        for t in self.listed:  # a cycle: a walk up that comes back
            seen, a = set(), t
            while a:
                if a in seen:
                    raise Format(listed_on[a], f"TaxID {a} is its own ancestor")
                seen.add(a)
                a = self.parent[a]
        self._chains = {}
        self.max_depth = max((self.depth(t) for t in self.parent), default=0)

    def parent_of(self, t):
        return self.parent.get(t, 0)

    def rank_code(self, t):
        return self.rank_names.index(self.rank[t].encode()) if t in self.rank else U32

    def rank_name(self, t):
        return self.rank.get(t, UNKNOWN)

    def chain(self, t):
        """t, its parent, ... , 0 (the callers do not change the list)"""
        if self._chains is not None and t in self._chains:
            return self._chains[t]
        out = [t]
        while out[-1]:
            out.append(self.parent_of(out[-1]))
        if self._chains is not None:
            self._chains[t] = out
        return out

    def depth(self, t):
        return len(self.chain(t)) - 1

    def lca(self, taxa):
        """the deepest node that is an ancestor-or-self of every member: the chains intersected"""
        taxa = list(taxa)
        common = set(self.chain(taxa[0]))
        for t in taxa[1:]:
            common &= set(self.chain(t))
        return max(common, key=self.depth)

    def lca_by_intervals(self, taxa):
        """the form the device uses: nodes numbered in preorder (children ascending by TaxID), a walk up from the member with the
        smallest number until the node's subtree holds the one with the largest"""
        nodes = set()
        for t in taxa:
            nodes.update(self.chain(t))
        kids = {}
        for t in nodes:
            if t:
                kids.setdefault(self.parent_of(t), []).append(t)
        num, last, order = {}, {}, []

        def visit(t):
            num[t] = len(order)
            order.append(t)
            for k in sorted(kids.get(t, [])):
                visit(k)
            last[t] = len(order) - 1

        visit(0)
        lo = min(taxa, key=num.get)
        hi = max(num[t] for t in taxa)
        while last[lo] < hi:
            lo = self.parent_of(lo)
        return lo


def entering(recs, slack):
    """the TaxIDs of one read's records whose edit is within slack of the smallest, and that smallest edit"""
    m = min(r[-1] for r in recs)
    bound = min(m + slack, U32)
    return sorted({r[1] for r in recs if r[-1] <= bound}), m


def per_read(tx, records, slack):
    """[(read, LCA TaxID, smallest edit)] in read order"""
    by_read = {}
    for r in records:
        by_read.setdefault(r[0], []).append(r)
    out = []
    for read in sorted(by_read):
        taxa, m = entering(by_read[read], slack)
        out.append((read, tx.lca(taxa), m))
    return out


def clade_rows(tx, lcas):
    """[(tax_id, parent, rank name, rank code, depth, direct, clade)] for the nodes with clade > 0, in preorder: every read's LCA
    walked to the root"""
    direct, clade = {}, {}
    for _, t, _ in lcas:
        direct[t] = direct.get(t, 0) + 1
        for a in tx.chain(t):
            clade[a] = clade.get(a, 0) + 1
    kids = {}
    for t in clade:
        if t:
            kids.setdefault(tx.parent_of(t), []).append(t)
    rows = []

    def visit(t):
        rows.append((t, tx.parent_of(t), tx.rank_name(t), tx.rank_code(t), tx.depth(t), direct.get(t, 0), clade[t]))
        for k in sorted(kids.get(t, [])):
            visit(k)

    if clade:
        visit(0)
    return rows


def report_text(rows, total_reads):
    denom = float(max(total_reads, 1))
    out = [HEADER]
    for t, p, rank, _, depth, direct, clade in rows:
        out.append("%d\t%d\t%s\t%d\t%d\t%.2f\t%d\t%.2f\n" % (t, p, rank, depth, direct, direct / denom * 100.0, clade, clade / denom * 100.0))
    return "".join(out).encode()


def lca_lines(lcas, read_ids):
    """the results text of the per-read records: READ_ID:LCA=EDIT"""
    return "".join(f"{read_ids[r]}:{t}={e}\n" for r, t, e in lcas).encode()
