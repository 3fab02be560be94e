"""Plain model of the ends-free engine's extension mode (include/saln.h,
SALN_MODE_EXTEND = 8): the alignment is pinned at the
origin and free at its end.  Written fresh; the GPU tests compare the engine
against it record for record and word for word, test_extend_model.py pins it
against brute-force enumeration.

q = query = columns j (length n), d = db = rows i (length m).  Scoring is
ends_free_sub_model.Scoring: s(i, j) = S[d[i-1]][q[j-1]], a function of the two
bytes, so one model serves scalar and matrix scoring.  Gaps open from M only;
a gap of length L costs o + L e.

    I(i,j) = max(I(i,j-1) + e, M(i,j-1) + o + e)      j >= 1
    D(i,j) = max(D(i-1,j) + e, M(i-1,j) + o + e)      i >= 1
    M(i,j) = s(i,j) + P(i-1,j-1)                      i, j >= 1
    P = max(M, I, D), no floor

M(0,0) = 0 is the only start and everything else no rule gives is -infinity.
The rules then give the borders I(0,j) = o + j e and D(i,0) = o + i e, and
I(i,1) = D(1,j) = -infinity: nothing opens from a border gap.

Score = max(0, max over i, j >= 1 of M(i,j)), the smallest i, then the smallest
j, winning a tie; nothing strictly positive: the empty alignment (score 0, no
words, coordinates 0).  The walk starts in M at the end cell; a diagonal step
that lands on row 0 is followed by one run of 'I' back to (0,0), one that
lands on column 0 by one run of 'D'.
"""
from __future__ import annotations

import numpy as np

from ends_free_model import NEG, Alignment, cigar_words  # noqa: F401  (re-exported)
from ends_free_sub_model import Scoring, matrix_scoring, scalar_scoring  # noqa: F401

EXTEND = 8
_REAL = -(1 << 59)        # everything below is -infinity


def _real(v):
    return np.where(v > _REAL, v, NEG)


def _next_row(M, I, D, s, o, e, j):
    """Row i of the three matrices from row i - 1 (M, I, D) and s = s(i, 1..n)."""
    P = np.maximum(np.maximum(M, I), D)
    Mn = np.full(len(M), NEG, np.int64)                      # M(i, 0) is -infinity
    Mn[1:] = _real(P[:-1] + s)
    Dn = _real(np.maximum(D + e, M + o + e))                 # column 0: D(i, 0) = o + i e
    In = np.full(len(M), NEG, np.int64)                      # I(i, 0) is -infinity
    if len(M) > 1:
        # I(i, j) = j e + max over j' < j of (M(i, j') + o - j' e)
        run = np.maximum.accumulate(_real(Mn + o - j * e))[:-1]
        In[1:] = _real(run + j[1:] * e)
    return Mn, In, Dn


def _row0(n, o, e):
    j = np.arange(n + 1, dtype=np.int64)
    M = np.full(n + 1, NEG, np.int64)
    M[0] = 0
    I = np.full(n + 1, NEG, np.int64)
    I[1:] = o + j[1:] * e
    return M, I, np.full(n + 1, NEG, np.int64), j


def fill(q: bytes, d: bytes, sc: Scoring):
    """The three matrices, (m+1) x (n+1) int64, -infinity as NEG."""
    n, m = len(q), len(d)
    qa = np.frombuffer(bytes(q), np.uint8)
    M, I, D = (np.full((m + 1, n + 1), NEG, np.int64) for _ in range(3))
    M[0], I[0], D[0], j = _row0(n, sc.o, sc.e)
    for i in range(1, m + 1):
        M[i], I[i], D[i] = _next_row(M[i - 1], I[i - 1], D[i - 1], sc.S[d[i - 1]][qa], sc.o, sc.e, j)
    return M, I, D


def align(q: bytes, d: bytes, sc: Scoring, walk: bool = True, path: list = None) -> Alignment:
    """path (optional): filled with the cells (i, j) the walk stands on, the
    end cell first, (0, 0) last."""
    assert sc.o <= 0 and sc.e < 0
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    z = 0 if walk else -1
    if n == 0 or m == 0:
        return Alignment(0, z, 0, z, 0)
    M, I, D = fill(q, d, sc)
    inner = M[1:, 1:]
    score = int(inner.max())
    if score <= 0:
        return Alignment(0, z, 0, z, 0)
    # the smallest i, then the smallest j: the first maximum in row-major order
    i, jj = (int(v) + 1 for v in np.unravel_index(int(np.argmax(inner)), inner.shape))
    end_i, end_j = i, jj
    if not walk:
        return Alignment(score, -1, end_j, -1, end_i)
    mats = (("M", M), ("I", I), ("D", D))
    st, ops = "M", []      # ops back to front
    while True:
        if path is not None:
            path.append((i, jj))
        if i == 0 and jj == 0:
            break
        if i == 0:                       # row 0: the rest of the query is one insertion
            ops.append("I")
            jj -= 1
        elif jj == 0:                    # column 0: the rest of the db is one deletion
            ops.append("D")
            i -= 1
        elif st == "M":
            ops.append("=" if q[jj - 1] == d[i - 1] else "X")
            v = int(M[i, jj]) - int(sc.S[d[i - 1]][q[jj - 1]])
            i, jj = i - 1, jj - 1
            if i == 0 or jj == 0:
                assert v == (0 if i == jj else o + (i + jj) * e)   # the border's P
            else:
                st = next(name for name, X in mats if int(X[i, jj]) == v)
        elif st == "I":
            ops.append("I")
            cur = int(I[i, jj])
            jj -= 1
            st = "I" if int(I[i, jj]) > _REAL and int(I[i, jj]) + e == cur else "M"   # extend before open
            assert st == "I" or int(M[i, jj]) + o + e == cur
        else:
            ops.append("D")
            cur = int(D[i, jj])
            i -= 1
            st = "D" if int(D[i, jj]) > _REAL and int(D[i, jj]) + e == cur else "M"
            assert st == "D" or int(M[i, jj]) + o + e == cur
    ops.reverse()
    cigar = []
    for op in ops:
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return Alignment(score, 0, end_j, 0, end_i, cigar)


def linear_ends(q: bytes, d: bytes, sc: Scoring):
    """(score, q_end, db_end) of align(..., walk=False) with rolling rows, for
    dbs whose full matrices would take gigabytes."""
    n, m = len(q), len(d)
    if n == 0 or m == 0:
        return 0, 0, 0
    qa = np.frombuffer(bytes(q), np.uint8)
    M, I, D, j = _row0(n, sc.o, sc.e)
    best, best_i, best_j = 0, 0, 0
    for i in range(1, m + 1):
        M, I, D = _next_row(M, I, D, sc.S[d[i - 1]][qa], sc.o, sc.e, j)
        jj = int(np.argmax(M[1:])) + 1        # the smallest j of the row
        if int(M[jj]) > best:                 # strict: the smallest row
            best, best_i, best_j = int(M[jj]), i, jj
    return best, best_j, best_i


def left_coords(a: Alignment, n: int, m: int) -> Alignment:
    """The alignment `a` of the two reversed sequences (lengths n, m) as
    extend_align(..., direction="left") reports it: the CIGAR reversed, the
    coordinates counted on the sequences as given."""
    return Alignment(a.score, n - a.q_end, n, m - a.db_end, m, list(a.cigar)[::-1])
