"""Plain model of the ends-free engine (include/saln.h, saln_ends_free_*):
local and semi-global Gotoh affine-gap alignment, exactly as DESIGN.md
section 3 defines them.  The GPU tests compare the engine against it record
for record and word for word; test_ends_free_model.py pins it against
brute-force enumeration.

q = query = columns j (length n), d = db = rows i (length m).  Gaps open from
M only; a gap of length L costs o + L e.

    I(i,j) = max(I(i,j-1) + e, M(i,j-1) + o + e)      j >= 1
    D(i,j) = max(D(i-1,j) + e, M(i-1,j) + o + e)      i >= 1
    M(i,j) = s(i,j) + P(i-1,j-1)                      i, j >= 1
    P = max(M, I, D) (semi-global), max(0, M, I, D) (local)

The fill is vectorised by rows: I of a row is a running maximum,
I(i,j) = j e + max over j' < j of (M(i,j') + o - j' e).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LOCAL, SEMI_GLOBAL = 1, 2
DEFAULT_SCORING = (5, -4, -8, -6)
NEG = -(1 << 60)          # -infinity
_REAL = -(1 << 59)        # everything below is -infinity


@dataclass
class Alignment:
    score: int
    q_begin: int
    q_end: int
    db_begin: int
    db_end: int
    cigar: list = field(default_factory=list)   # [(length, op)], forward order

    def record(self, status: int = 0):
        """(score, status, q_begin, q_end, db_begin, db_end, cigar_len, reserved)"""
        return (self.score, status, self.q_begin, self.q_end, self.db_begin, self.db_end,
                len(self.cigar), 0)


def fill(q: bytes, d: bytes, mode: int, scoring=None):
    """The three matrices, (m+1) x (n+1) int64, -infinity as NEG."""
    ma, mi, o, e = scoring if scoring is not None else DEFAULT_SCORING
    n, m = len(q), len(d)
    qa = np.frombuffer(bytes(q), np.uint8)
    M = np.full((m + 1, n + 1), NEG, np.int64)
    I = np.full((m + 1, n + 1), NEG, np.int64)
    D = np.full((m + 1, n + 1), NEG, np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    if mode == SEMI_GLOBAL:
        M[:, 0] = 0
    for i in range(m + 1):
        if i >= 1:
            P = np.maximum(np.maximum(M[i - 1], I[i - 1]), D[i - 1])
            if mode == LOCAL:
                P = np.maximum(P, 0)
            s = np.where(qa == d[i - 1], ma, mi).astype(np.int64)
            M[i, 1:] = np.where(P[:-1] > _REAL, P[:-1] + s, NEG)
            Dn = np.maximum(D[i - 1] + e, M[i - 1] + o + e)
            if mode == SEMI_GLOBAL:
                Dn[0] = NEG   # D(i, 0) is -infinity
            D[i] = np.where(Dn > _REAL, Dn, NEG)
        # I(i, j) for j >= 1 from M(i, j' < j)
        if n:
            t = np.where(M[i] > _REAL, M[i] + o - j * e, NEG)
            run = np.maximum.accumulate(t)[:-1]
            I[i, 1:] = np.where(run > _REAL, run + j[1:] * e, NEG)
    return M, I, D


def align(q: bytes, d: bytes, mode: int, scoring=None, walk: bool = True) -> Alignment:
    ma, mi, o, e = scoring if scoring is not None else DEFAULT_SCORING
    assert ma > 0 and mi < 0 and o <= 0 and e < 0
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    M, I, D = fill(q, d, mode, scoring)
    if mode == SEMI_GLOBAL:
        col = np.maximum(M[:, n], I[:, n])
        i = int(np.argmax(col))           # the smallest i among the maxima
        score = int(col[i])
        st = "M" if M[i, n] >= I[i, n] else "I"   # M before I
        jj = n
    else:
        best = int(M.max()) if n and m else NEG
        if best <= 0:
            z = 0 if walk else -1
            return Alignment(0, z, 0, z, 0)
        # the smallest i, then the smallest j: the first maximum in row-major order
        i, jj = (int(v) for v in np.unravel_index(int(np.argmax(M)), M.shape))
        score, st = best, "M"
    end_i, end_j = i, jj
    if not walk:
        return Alignment(score, -1, end_j, -1, end_i)
    ops = []   # back to front
    while True:
        if st == "M":
            if jj == 0:          # semi-global: column 0 is the start
                break
            sc = ma if q[jj - 1] == d[i - 1] else mi
            ops.append("=" if q[jj - 1] == d[i - 1] else "X")
            v = int(M[i, jj]) - sc
            i, jj = i - 1, jj - 1
            if mode == LOCAL:
                if v == 0:
                    break
            elif jj == 0:
                break
            for name, X in (("M", M), ("I", I), ("D", D)):
                if int(X[i, jj]) == v:
                    st = name
                    break
            else:
                raise AssertionError("walk: no predecessor")
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


def cigar_words(cigar) -> list:
    code = {"=": 7, "X": 8, "I": 1, "D": 2}
    return [(n << 4) | code[op] for n, op in cigar]


def tied_ends(q: bytes, d: bytes, mode: int, scoring=None):
    """(end cells holding the best value, distinct rows among them): what
    a reduction that ignores the tie rule could get wrong."""
    n, m = len(q), len(d)
    M, I, D = fill(q, d, mode, scoring)
    if mode == SEMI_GLOBAL:
        col = np.maximum(M[:, n], I[:, n])
        rows = np.nonzero(col == col.max())[0]
        return len(rows), len(rows)
    if not (n and m) or M.max() <= 0:
        return 0, 0
    ii, _ = np.nonzero(M == M.max())
    return len(ii), len(set(ii.tolist()))
