"""Result text back into assignment records, restated in Python (no library code): shared by test_parse_text_cpu.py and
test_parse_text.py.  Written from the description of mtsv_fold_add_text in include/mtsv_amd.h and from the rules of
mtsv-collapse (csrc/collapse_main.cpp), not from the kernels.

A call is a list of lines (read, hits): `hits` is the part of a result line behind its last ':', TOKEN(,TOKEN)* or nothing.
A token is T=E, T-G=E or T-G-O=E, every number 1 to 10 decimal digits with value <= 2^32 - 1.  records() gives the list of
the grain (tuples as fold_ref uses them): a run of adjacent tokens of one line with the same key becomes one record with the
smallest edit (TAXID_GI: the smallest (edit, offset)).  Refusals, in the order the library makes them:

  Format(line)  the first line with a token outside the grammar or, in a wide grain, without GI and offset
  Arg(line)     the first line whose keys descend, whose read is not above the previous non-empty line's, or whose read is
                at or above n_reads

collapse_files() is mtsv-collapse as the device path does it: lines cut by the tool's rules, the distinct IDs in byte order
as the dictionary, a file that names an ID on several lines cut into layers, every layer parsed, everything folded."""
import fold_ref as F

TAXID, TAXID_GI, LONG = F.TAXID, F.TAXID_GI, F.LONG
U32 = 2 ** 32 - 1


class Format(Exception):
    def __init__(self, line):
        super().__init__(f"line {line}")
        self.line = line


class Arg(Exception):
    def __init__(self, line):
        super().__init__(f"line {line}")
        self.line = line


def number(s):
    if not 1 <= len(s) <= 10 or any(c not in "0123456789" for c in s):
        return None
    v = int(s)
    return v if v <= U32 else None


def token(tok):
    """(tax, gi, offset, edit, fields on the left) or None"""
    if tok.count("=") != 1:
        return None
    left, right = tok.split("=")
    parts = left.split("-")
    nums = [number(p) for p in parts] + [number(right)]
    if len(parts) > 3 or None in nums:
        return None
    tax, gi, off = (nums[:-1] + [0, 0])[:3]
    return tax, gi, off, nums[-1], len(parts)


def key_of(grain, t):
    return t[:1] if grain == TAXID else t[:2] if grain == TAXID_GI else t[:3]


def records(grain, lines, n_reads):
    parsed = []
    for j, (read, hits) in enumerate(lines):
        toks = []
        if hits != "":
            for tok in hits.split(","):
                t = token(tok)
                if t is None or (grain != TAXID and t[4] != 3):
                    raise Format(j)
                toks.append(t)
        parsed.append(toks)
    prev_read = None
    for j, (read, _) in enumerate(lines):
        toks = parsed[j]
        if not toks:
            continue
        keys = [key_of(grain, t) for t in toks]
        if any(b < a for a, b in zip(keys, keys[1:])) or (prev_read is not None and read <= prev_read) or read >= n_reads:
            raise Arg(j)
        prev_read = read
    out = []
    for j, (read, _) in enumerate(lines):
        run_key, best = None, None
        for t in parsed[j]:
            k = key_of(grain, t)
            if k != run_key:
                if run_key is not None:
                    out.append(best)
                run_key, best = k, None
            tax, gi, off, edit, _ = t
            if grain == TAXID:
                cand = (read, tax, edit)
                if best is None or edit < best[2]:
                    best = cand
            elif grain == LONG:
                if best is None or edit < best[4]:
                    best = (read, tax, gi, off, edit)
            else:
                if best is None or (edit, off) < (best[4], best[3]):
                    best = (read, tax, gi, off, edit)
        if run_key is not None:
            out.append(best)
    return out


def arrays(lines):
    """(hits bytes, line_off, line_read) of a call, as mtsv_fold_add_text takes them"""
    import numpy as np
    blob = "".join(h for _, h in lines).encode("latin-1")
    off = np.zeros(len(lines) + 1, dtype=np.uint64)
    if lines:
        np.cumsum([len(h.encode("latin-1")) for _, h in lines], out=off[1:])
    return blob, off, np.array([r for r, _ in lines], dtype=np.uint32)


def split_text(text):
    """[(id, hits)] of a results file by mtsv-collapse's rules; ValueError for a line without ':' or with an empty ID"""
    out = []
    for l in text.split("\n"):
        l = l.rstrip("\r\n")
        if l.strip(" \t") == "":
            continue
        c = l.rfind(":")
        if c <= 0:
            raise ValueError(l)
        out.append((l[:c], l[c + 1:]))
    return out


def layers(file_lines, rank):
    """a file's lines [(id, hits)] as calls: layer k holds the k-th line of every ID, ordered by read number"""
    seen, out = {}, []
    for i, h in file_lines:
        k = seen.get(i, 0)
        seen[i] = k + 1
        while len(out) <= k:
            out.append([])
        out[k].append((rank[i], h))
    return [sorted(l, key=lambda x: x[0]) for l in out]


def collapse_files(grain, texts):
    """(ids in dictionary order, the folded records) of result files given as str"""
    files = [split_text(t) for t in texts]
    ids = sorted({i for f in files for i, _ in f}, key=lambda s: s.encode("latin-1"))
    rank = {s: k for k, s in enumerate(ids)}
    lists = [records(grain, call, len(ids)) for f in files for call in layers(f, rank)]
    return ids, F.fold_all(grain, lists)
