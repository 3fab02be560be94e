"""Plain model of the ends-free engine (include/saln.h, saln_ends_free_*,
saln_ends_free_sub_*): local, semi-global, overlap (dovetail) and extension
Gotoh affine-gap alignment under scalar or substitution-matrix scoring, exactly
as DESIGN.md sections 3 (3c), 3f and 3g define them.  One fill, one end-cell
rule and one walk serve the four modes.  The reference implements none of
them, so this file is the written definition: the GPU tests compare the engine
against it record for record and word for word; test_ends_free_model.py,
test_overlap_model.py, test_ends_free_sub_model.py and test_extend_model.py pin
it against brute-force enumeration and against tests/golden/
ends_free_model_pins.json.

q = query = columns j (length n), d = db = rows i (length m).  Gaps open from
M only (an I run and a D run are never adjacent); a gap of length L costs
o + L e.

    s(i,j) = S[d[i-1]][q[j-1]]     row: the db byte, column: the query byte
    I(i,j) = max(I(i,j-1) + e, M(i,j-1) + o + e)      j >= 1
    D(i,j) = max(D(i-1,j) + e, M(i-1,j) + o + e)      i >= 1
    M(i,j) = s(i,j) + P(i-1,j-1)                      i, j >= 1
    P = max(M, I, D); local: max(0, M, I, D)

A scalar scheme (ma, mi, o, e) is the S with ma on the diagonal and mi off it.
'=' and 'X' are byte comparisons, whatever the two bytes score.  The fill is
vectorised by rows: I of a row is a running maximum,
I(i,j) = j e + max over j' < j of (M(i,j') + o - j' e).

Borders (everything no rule gives is -infinity), end cell and walk stop:

LOCAL (1).  No border cell is a start; the floor of P is.  Score = max(0, max
    M(i,j)); nothing strictly positive: the empty alignment (score 0, no words,
    coordinates 0).  Else the smallest i, then the smallest j, wins a tie, and
    the end state is M.  The walk stops after the diagonal step whose
    P(i-1,j-1) is 0, so an alignment begins and ends with '=' or 'X'.
SEMI_GLOBAL (2).  M(i,0) = 0, i in 0..m, every one a free start; D(i,0) =
    -infinity; the rules give I(0,j) = o + j e.  End candidates: max(M, I)
    (i,n), i in 0..m: the whole query, never ending in D.  The largest value,
    then the smallest i; M before I.  No empty form: the score may be
    negative.  The walk stops on column 0.
OVERLAP (4).  M(i,0) = 0, i in 0..m; M(0,j) = 0, j in 0..n, every one a free
    start; I(i,0), I(0,j), D(i,0), D(0,j) = -infinity, so I(i,1) = o + e (from
    M(i,0)) and D(1,j) = o + e (from M(0,j)).  End candidates: P(i,n),
    1 <= i <= m, and P(m,j), 1 <= j <= n.  Score = max(0, best candidate);
    nothing strictly positive: the empty alignment.  Else the largest value,
    then the smallest i, then the smallest j (a last-column cell above row m
    wins a tie against a last-row cell; in row m the smaller column does); the
    end state is the first of M, I, D equal to P there.  The walk stops as
    soon as it stands on row 0 or column 0.
EXTEND (8).  M(0,0) = 0 is the only start.  The rules then give the borders
    I(0,j) = o + j e and D(i,0) = o + i e, and I(i,1) = D(1,j) = -infinity:
    nothing opens from a border gap.  Score = max(0, max over i, j >= 1 of
    M(i,j)), the smallest i, then the smallest j, winning a tie; nothing
    strictly positive: the empty alignment.  The walk starts in M at the end
    cell and stops at (0,0): a diagonal step that lands on row 0 is followed
    by one run of 'I' back to the origin, one that lands on column 0 by one
    run of 'D'.

Every walk prefers the first of M, I, D holding a diagonal step's predecessor
value and, inside a gap, extending before opening.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

LOCAL, SEMI_GLOBAL, OVERLAP, EXTEND = 1, 2, 4, 8
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


def cigar_words(cigar) -> list:
    code = {"=": 7, "X": 8, "I": 1, "D": 2}
    return [(n << 4) | code[op] for n, op in cigar]


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


_scalar_cached = functools.lru_cache(maxsize=None)(scalar_scoring)


def _scoring(scoring) -> Scoring:
    """None (the default scheme), a 4-tuple (ma, mi, o, e) or a Scoring."""
    sc = scoring if isinstance(scoring, Scoring) else _scalar_cached(*(scoring or DEFAULT_SCORING))
    assert sc.o <= 0 and sc.e < 0
    return sc


def _real(v):
    return np.where(v > _REAL, v, NEG)


def _rows(q: bytes, d: bytes, mode: int, sc: Scoring):
    """Rows 0..m of (M, I, D), n + 1 int64 each, -infinity as NEG.  One row
    step for the four modes, which differ in:

        row 0       M(0,0) = 0 but in local; M(0,j) = 0, j >= 1, in overlap
                    only; I(0,j) by its rule, but -infinity in overlap
        M(i,0)      0 in semi-global and overlap (a free start), else -infinity
        D(i,0)      forced to -infinity where M(i,0) = 0; else by its rule
                    (extend: o + i e; local: -infinity anyway)
        the floor   P = max(0, ...) in local only
    """
    o, e, n = sc.o, sc.e, len(q)
    qa = np.frombuffer(q, np.uint8)
    j = np.arange(n + 1, dtype=np.int64)
    neg = np.full(n + 1, NEG, np.int64)
    col0 = 0 if mode in (SEMI_GLOBAL, OVERLAP) else NEG

    def i_row(M):
        # -infinity stays far below everything real through the running maximum
        # and comes out at NEG or below; so does D's below
        I = neg.copy()
        if n:
            I[1:] = np.maximum(np.maximum.accumulate(M + (o - j * e))[:-1] + j[1:] * e, NEG)
        return I

    M = neg.copy()
    if mode != LOCAL:
        M[0] = 0
    if mode == OVERLAP:
        M[1:] = 0
    I, D = (neg if mode == OVERLAP else i_row(M)), neg
    yield M, I, D
    for c in d:
        P = np.maximum(np.maximum(M, I), D)
        if mode == LOCAL:
            P = np.maximum(P, 0)
        D = np.maximum(np.maximum(D + e, M + (o + e)), NEG)
        if col0 == 0:
            D[0] = NEG
        M = neg.copy()
        M[0] = col0
        M[1:] = _real(P[:-1] + sc.S[c][qa])
        I = i_row(M)
        yield M, I, D


def fill(q: bytes, d: bytes, mode: int, scoring=None):
    """The three matrices, (m+1) x (n+1) int64, -infinity as NEG."""
    return tuple(np.stack(X) for X in zip(*_rows(bytes(q), bytes(d), mode, _scoring(scoring))))


def _candidates(rows, mode, n, m):
    """Per row i that holds end candidates, (i, lo, V): V[k] is what an
    alignment ending at (i, lo + k) scores, rows as _rows gives them."""
    states = {LOCAL: 1, EXTEND: 1, SEMI_GLOBAL: 2, OVERLAP: 3}[mode]     # of M, I, D
    for i, row in enumerate(rows):
        # the last column only, or columns 1..n (local, extend, overlap's row m)
        lo = n if mode == SEMI_GLOBAL or (mode == OVERLAP and i < m) else 1
        if lo <= n:
            yield i, lo, functools.reduce(np.maximum, [X[lo:] for X in row[:states]]), row


def _end(rows, mode, n, m):
    """(score, i, j, state) of the end cell, or None for the empty alignment
    of local, overlap and extend.  Rows in order and strict >: the smallest i,
    then the smallest j; the state is the first of M, I, D there."""
    best, end = (NEG if mode == SEMI_GLOBAL else 0), None
    for i, lo, V, row in _candidates(rows, mode, n, m):
        k = int(np.argmax(V))                 # the smallest j among the row's maxima
        if int(V[k]) > best:
            best = int(V[k])
            end = best, i, lo + k, next(s for s, X in zip("MID", row) if int(X[lo + k]) == best)
    return end


def align(q: bytes, d: bytes, mode: int, scoring=None, walk: bool = True, path: list = None,
          info: dict = None) -> Alignment:
    """path (optional): filled with the cells (i, j) the walk stands on, the
    end cell first (local: the cell of the stop too).  info (optional, filled
    for a non-empty alignment): the end state 'st' and the candidates tied at
    the best value, 'col_ties' (rows i of (i, n)) and 'row_ties' (columns j of
    (m, j)): what the GPU tests assert about their overlap inputs."""
    sc = _scoring(scoring)
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    M, I, D = fill(q, d, mode, sc)
    end = _end(zip(M, I, D), mode, n, m)
    if end is None:
        z = 0 if walk else -1
        return Alignment(0, z, 0, z, 0)
    score, i, jj, st = end
    end_i, end_j = i, jj
    if info is not None:
        ties = _ties(M, I, D, mode, score)
        info.update(st=st, col_ties=[a for a, b in ties if b == n], row_ties=[b for a, b in ties if a == m])
    if not walk:
        return Alignment(score, -1, end_j, -1, end_i)
    mats = {"M": M, "I": I, "D": D}
    ops = []   # back to front
    while True:
        if path is not None:
            path.append((i, jj))
        if st == "M":
            if i == 0 or jj == 0:     # in M on a border: a start (extend: only (0,0) is real)
                break
            ops.append("=" if q[jj - 1] == d[i - 1] else "X")
            v = int(M[i, jj]) - int(sc.S[d[i - 1]][q[jj - 1]])
            i, jj = i - 1, jj - 1
            if mode == LOCAL and v == 0:          # the floor: the start
                if path is not None:
                    path.append((i, jj))
                break
            if mode == EXTEND and (i == 0 or jj == 0):
                assert v == (0 if i == jj else o + (i + jj) * e)   # the border's P
            st = next(s for s, X in mats.items() if int(X[i, jj]) == v)   # the first of M, I, D
        else:
            ops.append(st)
            X = mats[st]
            cur = int(X[i, jj])
            i, jj = (i, jj - 1) if st == "I" else (i - 1, jj)
            if not (int(X[i, jj]) > _REAL and int(X[i, jj]) + e == cur):   # extend before open
                assert int(M[i, jj]) + o + e == cur
                st = "M"
    cigar = []
    for op in reversed(ops):
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return Alignment(score, jj, end_j, i, end_i, cigar)


def linear_ends(q: bytes, d: bytes, mode: int, scoring=None):
    """(score, q_end, db_end) of align(..., walk=False) with rolling rows, for
    dbs whose full matrices would take gigabytes."""
    q, d = bytes(q), bytes(d)
    end = _end(_rows(q, d, mode, _scoring(scoring)), mode, len(q), len(d))
    return (0, 0, 0) if end is None else (end[0], end[2], end[1])


def _ties(M, I, D, mode, score):
    """The end candidates (i, j) that hold `score`, in row-major order."""
    m, n = M.shape[0] - 1, M.shape[1] - 1
    return [(i, lo + int(k)) for i, lo, V, _ in _candidates(zip(M, I, D), mode, n, m)
            for k in np.nonzero(V == score)[0]]


def tied_ends(q: bytes, d: bytes, mode: int, scoring=None):
    """(end cells holding the best value, distinct rows among them): what
    a reduction that ignores the tie rule could get wrong.  (0, 0) for the
    empty alignment."""
    M, I, D = fill(q, d, mode, scoring)
    end = _end(zip(M, I, D), mode, len(q), len(d))
    ties = _ties(M, I, D, mode, end[0]) if end else []
    return len(ties), len({i for i, _ in ties})


def end_info(q: bytes, d: bytes, scoring=None):
    """Overlap: align's info with the end cell ('i', 'j') and 'score', or None
    for the empty alignment."""
    info = {}
    a = align(q, d, OVERLAP, scoring, walk=False, info=info)
    if not info:
        return None
    info.update(score=a.score, i=a.db_end, j=a.q_end)
    return info


def left_coords(a: Alignment, n: int, m: int) -> Alignment:
    """The alignment `a` of the two reversed sequences (lengths n, m) as
    extend_align(..., direction="left") reports it: the CIGAR reversed, the
    coordinates counted on the sequences as given."""
    return Alignment(a.score, n - a.q_end, n, m - a.db_end, m, list(a.cigar)[::-1])
