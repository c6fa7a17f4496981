"""The plain restatement of a hit's placement (include/mtsv_amd.h, "alignments"), shared by test_place_cpu.py and
test_place.py.  Written from the definition in the header, not from the kernel: the semi-global matrix, column by column and
kept whole, the smallest end column within the hit's edit, and the traceback with its order of preference -- diagonal, up,
left."""
import collections

import numpy as np

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OP_CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}

Placed = collections.namedtuple("Placed", "start end cost ops")     # ops: [(length, op)] in reference order


def codes(seq):
    """A/a C/c G/g T/t -> 0..3, every other byte -> 4 (N)"""
    return np.array([_CODE.get(c, 4) for c in bytes(seq)], dtype=np.int64)


def strand_codes(read, strand):
    """the read's codes on a strand: forward, or reverse complement with N staying N"""
    c = codes(read)
    if strand:
        c = c[::-1]
        c = np.where(c < 4, 3 - c, c)
    return c


def matrix_until(P, T, edit):
    """the columns D[.][0], D[.][1], ... up to and including the first whose last entry is <= edit; (columns, end), end None when
    no column of T gets there.  D[0][j] = 0, D[i][0] = i, unit costs; a row matches a column iff the codes are equal and a base."""
    L = len(P)
    ar = np.arange(L + 1, dtype=np.int64)
    cols = [ar.copy()]
    if L <= edit:
        return cols, 0
    for j in range(1, len(T) + 1):
        t = T[j - 1]
        sub = np.where((P == t) & (P < 4), 0, 1)
        prev = cols[-1]
        tmp = np.empty(L + 1, dtype=np.int64)
        tmp[0] = 0
        tmp[1:] = np.minimum(prev[:-1] + sub, prev[1:] + 1)
        # D[i][j] = min(tmp[i], D[i-1][j] + 1): the smallest tmp[k] + (i - k) over k <= i
        cur = np.minimum.accumulate(tmp - ar) + ar
        cols.append(cur)
        if cur[L] <= edit:
            return cols, j
    return cols, None


def min_edit(P, T):
    """the smallest entry of the last row over every column of T: the edit a binner's hit over that window carries"""
    cols, _ = matrix_until(np.asarray(P, dtype=np.int64), np.asarray(T, dtype=np.int64), -1)
    return int(min(c[len(P)] for c in cols))


def place(P, T, edit):
    """P, T: code arrays (strand_codes / codes); None for an unplaceable hit"""
    P, T = np.asarray(P, dtype=np.int64), np.asarray(T, dtype=np.int64)
    D, end = matrix_until(P, T, edit)
    if end is None:
        return None
    i, j = len(P), end
    path = []
    while i > 0:
        match = j > 0 and P[i - 1] == T[j - 1] and P[i - 1] < 4
        if j > 0 and D[j - 1][i - 1] + (0 if match else 1) == D[j][i]:
            path.append(OP_EQ if match else OP_X)
            i, j = i - 1, j - 1
        elif D[j][i - 1] + 1 == D[j][i]:
            path.append(OP_I)
            i -= 1
        else:
            path.append(OP_D)
            j -= 1
    path.reverse()
    ops = []
    for op in path:
        if ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + 1, op)
        else:
            ops.append((1, op))
    return Placed(j, end, int(D[end][len(P)]), ops)


def place_hit(read, strand, bin_seq, offset, edit):
    """the hit's (ref_start, ref_end, ops), or None: bin_seq is the sequence of the hit's (tax_id, gi) as the index holds it"""
    got = place(strand_codes(read, strand), codes(bin_seq[offset:]), edit)
    if got is None:
        return None
    return offset + got.start, offset + got.end, got.ops


def encode(ops):
    return [length << 4 | op for length, op in ops]


def cigar(ops):
    return "".join(f"{length}{OP_CHAR[op]}" for length, op in ops) if ops else "*"


def line(read_id, tax_id, gi, strand, start, end, edit, ops):
    """the text of mtsv_format_placements for one placement"""
    return f"{read_id}\t{tax_id}\t{gi}\t{'-' if strand else '+'}\t{start}\t{end}\t{edit}\t{cigar(ops)}\n"


def check_cigar(P, T, placed, edit):
    """a script against its own definition; raises AssertionError"""
    i, j, cost = 0, placed.start, 0
    for length, op in placed.ops:
        assert length > 0 and op in OP_CHAR
        for _ in range(length):
            if op in (OP_EQ, OP_X):
                same = P[i] == T[j] and P[i] < 4
                assert same == (op == OP_EQ), (i, j, op)
                i, j = i + 1, j + 1
            elif op == OP_I:
                i += 1
            else:
                j += 1
            cost += op != OP_EQ
    assert i == len(P) and j == placed.end and cost == placed.cost <= edit, (i, j, cost, placed, edit)
    assert all(a[1] != b[1] for a, b in zip(placed.ops, placed.ops[1:])) and len(placed.ops) <= 2 * min(edit, len(P)) + 1
    assert placed.end - placed.start <= len(P) + min(edit, len(P))
