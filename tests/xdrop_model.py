"""Plain model of the X-drop extension (include/saln.h, "X-drop extension";
saln_ends_free_xdrop_*): the written definition, O(nm),
one cell at a time.  The GPU tests compare the engine against it record for
record and word for word; test_xdrop_model.py holds it to ends_free_model
(EXTEND) at large X, to other evaluation orders and to hand-derived cases.

Everything of ends_free_model's EXTEND stays (q = query = columns j, length n;
d = db = rows i, length m; borders, recurrences, tie rules, the walk).  Every
cell also carries B(i,j), the largest P of an unpruned cell in its dominance
region {(i',j') : i' <= i, j' <= j}:

    (0,0): P = B = 0, never pruned
    every other cell: M, I, D by the recurrences from its neighbours' values
        after pruning; P = max(M, I, D); Bin = max(B(i-1,j), B(i,j-1)), a B
        outside the matrix being -infinity
    pruned iff P < Bin - X (strict): then M = I = D = -infinity for every
        successor and B = Bin; else the values stay and B = max(Bin, P)

Score and end cell: max(0, max M(i,j) over the unpruned cells, i, j >= 1), the
smallest i, then the smallest j.  L is the last row that holds an unpruned
cell; every row below it is pruned throughout, which is why `fill` may stop
at the first row without one (stop=False computes every row; the tests
compare the two).
"""
from __future__ import annotations

import numpy as np

from ends_free_model import NEG, Alignment, Scoring, _scoring, cigar_words  # noqa: F401

_REAL = -(1 << 59)        # everything below is -infinity


def _plus(v: int, c: int) -> int:
    return v + c if v > _REAL else NEG


def cell(diagP: int, up, left, s: int, o: int, e: int, X: int):
    """One cell other than the origin: (M, I, D, B, alive) from P(i-1,j-1), the
    cell above and the cell to the left (each (M, I, D, B, alive), or None
    outside the matrix) and s(i,j) (None on row 0 and column 0)."""
    M = _plus(diagP, s) if s is not None else NEG
    I = max(_plus(left[1], e), _plus(left[0], o + e)) if left is not None else NEG
    D = max(_plus(up[2], e), _plus(up[0], o + e)) if up is not None else NEG
    P = max(M, I, D)
    Bin = max(up[3] if up is not None else NEG, left[3] if left is not None else NEG)
    if P < Bin - X:
        return NEG, NEG, NEG, Bin, False
    return M, I, D, max(Bin, P), True


ORIGIN = (0, NEG, NEG, 0, True)


def fill(q: bytes, d: bytes, X: int, scoring=None, stop: bool = True):
    """Rows 0 .. R of the cells, each a list of n + 1 (M, I, D, B, alive), in
    row-major order.  stop: R is the first row without an unpruned cell (or
    m); else R = m."""
    sc = _scoring(scoring)
    assert X >= 0
    o, e, n = sc.o, sc.e, len(q)
    rows = []
    for i in range(len(d) + 1):
        S = sc.S[d[i - 1]] if i else None
        up_row = rows[i - 1] if i else None
        row = []
        for j in range(n + 1):
            if i == 0 and j == 0:
                row.append(ORIGIN)
                continue
            up = up_row[j] if i else None
            left = row[j - 1] if j else None
            if i and j:
                dg = up_row[j - 1]
                c = cell(max(dg[0], dg[1], dg[2]), up, left, int(S[q[j - 1]]), o, e, X)
            else:
                c = cell(NEG, up, left, None, o, e, X)
            row.append(c)
        rows.append(row)
        if stop and not any(c[4] for c in row):
            break
    return rows


def align(q: bytes, d: bytes, X: int, scoring=None, walk: bool = True, path: list = None,
          stop: bool = True):
    """(Alignment, alive, L): the alignment as ends_free_model.align gives it
    (walk=False: begins -1, no CIGAR), the (m + 1) x (n + 1) mask of the
    unpruned cells, and the last row that holds one.  path (optional): the
    cells the walk stands on, the end cell first."""
    sc = _scoring(scoring)
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    rows = fill(q, d, X, sc, stop)
    alive = np.zeros((m + 1, n + 1), bool)
    for i, row in enumerate(rows):
        alive[i] = [c[4] for c in row]
    L = int(np.nonzero(alive.any(axis=1))[0][-1])
    best, end = 0, None
    for i in range(1, len(rows)):
        for j in range(1, n + 1):
            c = rows[i][j]
            if c[4] and c[0] > best:        # rows, then columns, rising: the smallest i, then j
                best, end = c[0], (i, j)
    if end is None:
        z = 0 if walk else -1
        return Alignment(0, z, 0, z, 0), alive, L
    end_i, end_j = end
    if not walk:
        return Alignment(best, -1, end_j, -1, end_i), alive, L
    i, j, st, ops = end_i, end_j, 0, []          # st: 0 M, 1 I, 2 D
    while True:
        assert rows[i][j][4], "the walk stands on a pruned cell"
        if path is not None:
            path.append((i, j))
        if st == 0:
            if i == 0 or j == 0:
                assert i == 0 and j == 0        # in M on a border: only the origin is real
                break
            ops.append("=" if q[j - 1] == d[i - 1] else "X")
            v = rows[i][j][0] - int(sc.S[d[i - 1]][q[j - 1]])
            i, j = i - 1, j - 1
            st = next(k for k in range(3) if rows[i][j][k] == v)      # the first of M, I, D
        else:
            ops.append("ID"[st - 1])
            cur = rows[i][j][st]
            i, j = (i, j - 1) if st == 1 else (i - 1, j)
            if not (rows[i][j][st] > _REAL and rows[i][j][st] + e == cur):   # extend before open
                assert rows[i][j][0] + o + e == cur
                st = 0
    cigar = []
    for op in reversed(ops):
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return Alignment(best, 0, end_j, 0, end_i, cigar), alive, L


def no_drop(n: int, m: int, scoring=None) -> int:
    """An X under which nothing real is pruned: 2 (n + m + 2) max|parameter|."""
    sc = _scoring(scoring)
    mx = max(int(np.abs(sc.S).max()), -sc.o, -sc.e)
    return 2 * (n + m + 2) * mx


def steps_bound(m: int, L: int, lanes: int) -> int:
    """The most row-loop steps a group of `lanes` lanes runs (the records'
    `reserved`): min(m, L) + lanes - 1 for the skew, and 1 for the vote, which
    the group takes after every step."""
    return min(m, L) + lanes - 1 + 1
