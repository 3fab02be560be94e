"""Plain model of the ends-free engine's overlap (dovetail) mode
(include/saln.h, SALN_MODE_OVERLAP), exactly as DESIGN.md section 3c defines
it.  The GPU tests compare the engine against it record for record and word
for word; test_overlap_model.py pins it against brute-force enumeration.

q = query = columns j (length n), d = db = rows i (length m).  Gaps open from
M only; a gap of length L costs o + L e.  The recurrences are
ends_free_model.py's with P = max(M, I, D) and no floor; the borders:

    M(i,0) = 0, i in 0..m;  M(0,j) = 0, j in 0..n      every one a free start
    I(i,0), I(0,j), D(i,0), D(0,j) = -infinity
    so I(i,1) = o + e (from M(i,0)) and D(1,j) = o + e (from M(0,j))

End candidates: P(i,n), 1 <= i <= m, and P(m,j), 1 <= j <= n.  Score = max(0,
best candidate); nothing strictly positive: the empty alignment (score 0, no
words, coordinates 0).  Else the largest value, then the smallest i, then the
smallest j; the end state is the first of M, I, D equal to P there.  The walk
stops as soon as it stands on row 0 or column 0.
"""
from __future__ import annotations

import numpy as np

from ends_free_model import NEG, Alignment, cigar_words  # noqa: F401  (re-exported)

OVERLAP = 4
DEFAULT_SCORING = (5, -4, -8, -6)
_REAL = -(1 << 59)        # everything below is -infinity


def _i_row(M, o, e, j):
    """I(i, j) for j >= 1 from M(i, j' < j): j e + max over j' < j of (M(i,j') + o - j' e)."""
    I = np.full(len(M), NEG, np.int64)
    if len(M) > 1:
        run = np.maximum.accumulate(M + o - j * e)[:-1]
        I[1:] = run + j[1:] * e
    return I


def fill(q: bytes, d: bytes, scoring=None):
    """The three matrices, (m+1) x (n+1) int64, -infinity as NEG."""
    ma, mi, o, e = scoring if scoring is not None else DEFAULT_SCORING
    n, m = len(q), len(d)
    qa = np.frombuffer(bytes(q), np.uint8)
    M = np.full((m + 1, n + 1), NEG, np.int64)
    I = np.full((m + 1, n + 1), NEG, np.int64)
    D = np.full((m + 1, n + 1), NEG, np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    M[:, 0] = 0
    M[0, :] = 0
    for i in range(1, m + 1):
        P = np.maximum(np.maximum(M[i - 1], I[i - 1]), D[i - 1])   # real everywhere: M(i-1, .) is
        M[i, 1:] = P[:-1] + np.where(qa == d[i - 1], ma, mi)
        Dn = np.maximum(D[i - 1] + e, M[i - 1] + o + e)
        Dn[0] = NEG                                                # D(i, 0) is -infinity
        D[i] = np.where(Dn > _REAL, Dn, NEG)
        I[i] = _i_row(M[i], o, e, j)                               # row 0's I stays -infinity
    return M, I, D


def _pick_end(col_vals, row_vals, m, n):
    """(value, i, j) of the end cell from P(1..m, n) and P(m, 1..n), or None
    when no candidate is strictly positive."""
    best, cell = 0, None
    if len(col_vals):
        i = int(np.argmax(col_vals))          # the smallest i among the maxima
        if int(col_vals[i]) > 0:
            best, cell = int(col_vals[i]), (i + 1, n)
    if len(row_vals):
        j = int(np.argmax(row_vals))          # the smallest j among the maxima
        v = int(row_vals[j])
        # a last-column cell above row m wins a tie; in row m the smaller column does
        if v > best or (v == best and v > 0 and cell[0] == m):
            best, cell = v, (m, j + 1)
    return None if cell is None else (best,) + cell


def align(q: bytes, d: bytes, scoring=None, walk: bool = True, info: dict = None) -> Alignment:
    """info (optional, filled for a non-empty alignment): the end state 'st'
    and the candidates tied at the best value, 'col_ties' (rows i of (i, n))
    and 'row_ties' (columns j of (m, j)): what the GPU tests assert about
    their inputs."""
    ma, mi, o, e = scoring if scoring is not None else DEFAULT_SCORING
    assert ma > 0 and mi < 0 and o <= 0 and e < 0
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    z = 0 if walk else -1
    if n == 0 or m == 0:
        return Alignment(0, z, 0, z, 0)
    M, I, D = fill(q, d, scoring)
    P = np.maximum(np.maximum(M, I), D)
    end = _pick_end(P[1:, n], P[m, 1:], m, n)
    if end is None:
        return Alignment(0, z, 0, z, 0)
    score, i, jj = end
    end_i, end_j = i, jj
    mats = (("M", M), ("I", I), ("D", D))
    st = next(name for name, X in mats if int(X[i, jj]) == score)   # the first of M, I, D
    if info is not None:
        info.update(st=st, col_ties=(np.nonzero(P[1:, n] == score)[0] + 1).tolist(),
                    row_ties=(np.nonzero(P[m, 1:] == score)[0] + 1).tolist())
    if not walk:
        return Alignment(score, -1, end_j, -1, end_i)
    ops = []   # back to front
    while i > 0 and jj > 0:
        if st == "M":
            same = q[jj - 1] == d[i - 1]
            ops.append("=" if same else "X")
            v = int(M[i, jj]) - (ma if same else mi)
            i, jj = i - 1, jj - 1
            if i == 0 or jj == 0:
                assert v == 0
                break
            st = next(name for name, X in mats if int(X[i, jj]) == v)
        elif st == "I":
            ops.append("I")
            cur = int(I[i, jj])
            jj -= 1
            st = "I" if int(I[i, jj]) > _REAL and int(I[i, jj]) + e == cur else "M"   # extend before open
            if st == "M":
                assert int(M[i, jj]) + o + e == cur
        else:
            ops.append("D")
            cur = int(D[i, jj])
            i -= 1
            st = "D" if int(D[i, jj]) > _REAL and int(D[i, jj]) + e == cur else "M"
            if st == "M":
                assert int(M[i, jj]) + o + e == cur
    ops.reverse()
    cigar = []
    for op in ops:
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return Alignment(score, jj, end_j, i, end_i, cigar)


def end_info(q: bytes, d: bytes, scoring=None):
    """align's info with the end cell ('i', 'j') and 'score', or None for the
    empty alignment."""
    info = {}
    a = align(q, d, scoring, walk=False, info=info)
    if not info:
        return None
    info.update(score=a.score, i=a.db_end, j=a.q_end)
    return info


def linear_ends(q: bytes, d: bytes, scoring=None):
    """(score, q_end, db_end) of align(..., walk=False) with rolling rows, for
    dbs whose full matrices would take gigabytes."""
    ma, mi, o, e = scoring if scoring is not None else DEFAULT_SCORING
    n, m = len(q), len(d)
    if n == 0 or m == 0:
        return 0, 0, 0
    qa = np.frombuffer(bytes(q), np.uint8)
    da = np.frombuffer(bytes(d), np.uint8)
    j = np.arange(n + 1, dtype=np.int64)
    M = np.zeros(n + 1, np.int64)
    I = np.full(n + 1, NEG, np.int64)
    D = np.full(n + 1, NEG, np.int64)
    best, best_i = 0, 0       # the last column, strict >: the smallest row
    for i in range(1, m + 1):
        P = np.maximum(np.maximum(M, I), D)
        D = np.maximum(D + e, M + (o + e))
        D[0] = NEG
        Mn = np.empty(n + 1, np.int64)
        Mn[0] = 0
        Mn[1:] = P[:-1] + np.where(qa == da[i - 1], ma, mi)
        M = Mn
        I = _i_row(M, o, e, j)
        v = int(max(M[n], I[n], D[n]))
        if v > best:
            best, best_i = v, i
    P = np.maximum(np.maximum(M, I), D)
    jj = int(np.argmax(P[1:])) + 1
    v = int(P[jj])
    if v > best or (v == best and v > 0 and best_i == m):
        return v, jj, m
    if best > 0:
        return best, n, best_i
    return 0, 0, 0
