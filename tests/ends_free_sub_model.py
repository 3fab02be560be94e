"""Plain model of the ends-free engine under a substitution matrix
(include/saln.h, saln_ends_free_sub_*): local, semi-global and overlap Gotoh
affine-gap alignment with s(i, j) a function of the two bytes,

    s(i, j) = S[d[i-1]][q[j-1]]          row: the db byte, column: the query byte

and everything else as ends_free_model.py and overlap_model.py have it (written
fresh here, one fill and one walk for the three modes; those two files are the
checkers of the scalar scoring and stay as they are).  The GPU tests compare
the engine against it record for record and word for word;
test_ends_free_sub_model.py pins it against brute-force enumeration and
against the two scalar models.

q = query = columns j (length n), d = db = rows i (length m).  Gaps open from
M only; a gap of length L costs o + L e.

    I(i,j) = max(I(i,j-1) + e, M(i,j-1) + o + e)      j >= 1
    D(i,j) = max(D(i-1,j) + e, M(i-1,j) + o + e)      i >= 1
    M(i,j) = s(i,j) + P(i-1,j-1)                      i, j >= 1
    P = max(M, I, D) (semi-global, overlap), max(0, M, I, D) (local)

Borders: semi-global M(i,0) = 0; overlap M(i,0) = M(0,j) = 0 with I(0,j) and
D(i,0) -infinity; everything no rule gives is -infinity.  '=' and 'X' are byte
comparisons, whatever the two bytes score.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ends_free_model import NEG, Alignment, cigar_words  # noqa: F401  (re-exported)

LOCAL, SEMI_GLOBAL, OVERLAP = 1, 2, 4
_REAL = -(1 << 59)        # everything below is -infinity


@dataclass
class Scoring:
    S: np.ndarray         # 256 x 256 int64: S[db byte][query byte]
    o: int
    e: int


def scalar_scoring(ma: int, mi: int, o: int, e: int) -> Scoring:
    """The scalar scheme as a function of the two bytes."""
    return Scoring(np.where(np.eye(256, dtype=bool), ma, mi).astype(np.int64), o, e)


def matrix_scoring(alphabet: bytes, scores, o: int, e: int, unknown=None,
                   case_insensitive: bool = False) -> Scoring:
    """scores[a][b]: the db symbol alphabet[a] against the query symbol
    alphabet[b].  A byte outside the alphabet scores `unknown` (default: the
    smallest entry) against everything and everything against it."""
    t = np.asarray(scores, np.int64)
    n = len(alphabet)
    assert t.shape == (n, n)
    if unknown is None:
        unknown = int(t.min())
    S = np.full((256, 256), unknown, np.int64)
    for a, x in enumerate(alphabet):
        xs = {x, ord(chr(x).lower()), ord(chr(x).upper())} if case_insensitive else {x}
        for b, y in enumerate(alphabet):
            ys = {y, ord(chr(y).lower()), ord(chr(y).upper())} if case_insensitive else {y}
            for xx in xs:
                for yy in ys:
                    S[xx, yy] = t[a, b]
    return Scoring(S, o, e)


def fill(q: bytes, d: bytes, mode: int, sc: Scoring):
    """The three matrices, (m+1) x (n+1) int64, -infinity as NEG."""
    o, e = sc.o, sc.e
    n, m = len(q), len(d)
    qa = np.frombuffer(bytes(q), np.uint8)
    M = np.full((m + 1, n + 1), NEG, np.int64)
    I = np.full((m + 1, n + 1), NEG, np.int64)
    D = np.full((m + 1, n + 1), NEG, np.int64)
    j = np.arange(n + 1, dtype=np.int64)
    if mode in (SEMI_GLOBAL, OVERLAP):
        M[:, 0] = 0
    if mode == OVERLAP:
        M[0, :] = 0
    for i in range(m + 1):
        if i >= 1:
            P = np.maximum(np.maximum(M[i - 1], I[i - 1]), D[i - 1])
            if mode == LOCAL:
                P = np.maximum(P, 0)
            s = sc.S[d[i - 1]][qa]
            M[i, 1:] = np.where(P[:-1] > _REAL, P[:-1] + s, NEG)
            Dn = np.maximum(D[i - 1] + e, M[i - 1] + o + e)
            Dn[0] = NEG   # D(i, 0) is -infinity
            D[i] = np.where(Dn > _REAL, Dn, NEG)
        # I(i, j) for j >= 1 from M(i, j' < j); overlap's I(0, j) is -infinity
        if n and not (mode == OVERLAP and i == 0):
            t = np.where(M[i] > _REAL, M[i] + o - j * e, NEG)
            run = np.maximum.accumulate(t)[:-1]
            I[i, 1:] = np.where(run > _REAL, run + j[1:] * e, NEG)
    return M, I, D


def _end(M, I, D, mode, n, m):
    """(score, i, j, state) of the end cell, or None for the empty alignment
    of local and overlap."""
    if mode == SEMI_GLOBAL:
        col = np.maximum(M[:, n], I[:, n])
        i = int(np.argmax(col))               # the smallest i among the maxima
        return int(col[i]), i, n, ("M" if M[i, n] >= I[i, n] else "I")   # M before I
    if n == 0 or m == 0:
        return None
    if mode == LOCAL:
        best = int(M.max())
        if best <= 0:
            return None
        # the smallest i, then the smallest j: the first maximum in row-major order
        i, j = (int(v) for v in np.unravel_index(int(np.argmax(M)), M.shape))
        return best, i, j, "M"
    P = np.maximum(np.maximum(M, I), D)
    best, cell = 0, None
    i = int(np.argmax(P[1:, n])) + 1          # the smallest i among the maxima
    if int(P[i, n]) > 0:
        best, cell = int(P[i, n]), (i, n)
    j = int(np.argmax(P[m, 1:])) + 1          # the smallest j among the maxima
    v = int(P[m, j])
    # a last-column cell above row m wins a tie; in row m the smaller column does
    if v > best or (v == best and v > 0 and cell[0] == m):
        best, cell = v, (m, j)
    if cell is None:
        return None
    i, j = cell
    st = next(name for name, X in (("M", M), ("I", I), ("D", D)) if int(X[i, j]) == best)
    return best, i, j, st


def align(q: bytes, d: bytes, mode: int, sc: Scoring, walk: bool = True, path: list = None) -> Alignment:
    """path (optional): filled with the cells (i, j) the walk stands on, the
    end cell first."""
    assert sc.o <= 0 and sc.e < 0
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    M, I, D = fill(q, d, mode, sc)
    end = _end(M, I, D, mode, n, m)
    if end is None:
        z = 0 if walk else -1
        return Alignment(0, z, 0, z, 0)
    score, i, jj, st = end
    end_i, end_j = i, jj
    if not walk:
        return Alignment(score, -1, end_j, -1, end_i)
    mats = (("M", M), ("I", I), ("D", D))
    ops = []   # back to front
    while True:
        if path is not None:
            path.append((i, jj))
        if jj == 0 or (mode == OVERLAP and i == 0):
            break                # column 0 is the start; overlap: row 0 too
        if st == "M":
            ops.append("=" if q[jj - 1] == d[i - 1] else "X")
            v = int(M[i, jj]) - int(sc.S[d[i - 1]][q[jj - 1]])
            i, jj = i - 1, jj - 1
            if mode == LOCAL:
                if v == 0:
                    if path is not None:
                        path.append((i, jj))
                    break
            elif jj == 0 or (mode == OVERLAP and i == 0):
                continue
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


def linear_ends(q: bytes, d: bytes, mode: int, sc: Scoring):
    """(score, q_end, db_end) of align(..., walk=False) with rolling rows, for
    dbs whose full matrices would take gigabytes."""
    o, e = sc.o, sc.e
    n, m = len(q), len(d)
    if n == 0 or (m == 0 and mode != SEMI_GLOBAL):
        return 0, 0, 0
    qa = np.frombuffer(bytes(q), np.uint8)
    j = np.arange(n + 1, dtype=np.int64)

    def i_row(Mr):
        t = np.where(Mr > _REAL, Mr + o - j * e, NEG)
        run = np.maximum.accumulate(t)[:-1]
        out = np.full(n + 1, NEG, np.int64)
        out[1:] = np.where(run > _REAL, run + j[1:] * e, NEG)
        return out

    M = np.full(n + 1, NEG, np.int64)
    if mode == OVERLAP:
        M[:] = 0
    elif mode == SEMI_GLOBAL:
        M[0] = 0
    I = np.full(n + 1, NEG, np.int64) if mode == OVERLAP else i_row(M)
    D = np.full(n + 1, NEG, np.int64)
    if mode == SEMI_GLOBAL:
        best, best_i, best_j = int(max(M[n], I[n])), 0, n
    else:
        best, best_i, best_j = 0, 0, 0
    for i in range(1, m + 1):
        P = np.maximum(np.maximum(M, I), D)
        if mode == LOCAL:
            P = np.maximum(P, 0)
        Dn = np.maximum(D + e, M + (o + e))
        Dn[0] = NEG
        D = np.where(Dn > _REAL, Dn, NEG)
        Mn = np.full(n + 1, NEG, np.int64)
        if mode != LOCAL:
            Mn[0] = 0
        Mn[1:] = np.where(P[:-1] > _REAL, P[:-1] + sc.S[d[i - 1]][qa], NEG)
        M = Mn
        I = i_row(M)
        if mode == LOCAL:
            jj = int(np.argmax(M))            # the smallest j of the row
            if int(M[jj]) > best:             # strict: the smallest row
                best, best_i, best_j = int(M[jj]), i, jj
        elif mode == SEMI_GLOBAL:
            v = int(max(M[n], I[n]))
            if v > best:
                best, best_i = v, i
        else:
            v = int(max(M[n], I[n], D[n]))
            if v > best:
                best, best_i, best_j = v, i, n
    if mode == OVERLAP:
        P = np.maximum(np.maximum(M, I), D)
        jj = int(np.argmax(P[1:])) + 1
        v = int(P[jj])
        if v > best or (v == best and v > 0 and best_i == m):
            return v, jj, m
        return (best, n, best_i) if best > 0 else (0, 0, 0)
    if mode == LOCAL and best <= 0:
        return 0, 0, 0
    return best, best_j, best_i
