"""Plain model of the chunked X-drop fill's schedule (saln_ends_free_xdrop_long_*,
ends_free_xdrop_long_kernels.hip).  The definition is
xdrop_model's; this file evaluates it the way the kernel does, in chunks of W
query columns (the kernel's W is 1,024), each chunk over a window of rows only,
by the kernel's own rules:

  chunk 0 runs from row lo = 1 with B = 0 above it.  Chunk c > 0 with boundary
  column c0 = c W: if (0, c0) is unpruned (o + c0 e >= -X) it runs from lo = 1
  with B = 0 above it; else from lo = pf, the first row whose boundary cell
  chunk c - 1 published unpruned, with P = D = -inf and B = B(pf - 1, c0) above
  it in every column (the published entry of row pf - 1, or the B chunk c - 1
  itself started from when pf is its first row); without such a row the pair
  ends.  The boundary cell of a row r above z_p, the last row chunk c - 1
  published, is taken as pruned with B = 0 (its B(z_p, c0) is already in B(r - 1,
  c0 + 1), which the chunk computed): the entry of such a row is never read,
  and here reading one raises (the kernel's slot holds another chunk's or
  another pair's values there).  A row is alive if one of its
  cells in the chunk or its boundary cell is unpruned, or if it is at most z_p
  (c > 0); the chunk runs until the first row that is not, and z_c = min(m,
  max(last alive row, lo)) is the last row it publishes.

Nothing else is evaluated: `computed` marks the cells that were, and the tests
hold them to xdrop_model and every other cell to "pruned".
"""
from __future__ import annotations

import numpy as np

from ends_free_model import NEG, Alignment
from xdrop_model import _REAL, _plus, _scoring


def steps_bound(windows, lanes: int = 64) -> int:
    """The most row-loop steps a wave of `lanes` lanes runs on a pair (the
    record's `reserved`): per chunk that ran, with its window (a, z), the rows
    z - a + 1, lanes - 1 steps of skew, and 1 for the vote.  The kernel does not
    align a chunk's start to the refill period, so nothing is added for that."""
    return sum((z - a + 1) + (lanes - 1) + 1 for a, z in windows)


class _Slot(dict):
    """The boundary column of one wave: row -> (P(r, c0), I(r, c0 + 1), B(r, c0)).
    A row without an entry of the current chunk is poison."""

    def __missing__(self, r):
        raise AssertionError(f"boundary entry of row {r} read, but the chunk before did not publish it")


def schedule(q: bytes, d: bytes, X: int, scoring=None, W: int = 1024):
    """(cells, computed, windows, end): cells maps (i, j) to (M, I, D, B, alive)
    for every cell the schedule evaluated (row 0 and column 0 by their closed
    forms), computed is the (m + 1) x (n + 1) mask of those, windows the (lo, z)
    of every chunk that ran, in order, and end (score, i, j) the end cell as the
    kernel merges it from the chunks' bests."""
    sc = _scoring(scoring)
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    assert X >= 0 and W >= 1
    cells = {(0, 0): (0, NEG, NEG, 0, True)}
    for j in range(1, n + 1):
        v = o + j * e
        cells[0, j] = (NEG, v, NEG, 0, True) if v >= -X else (NEG, NEG, NEG, 0, False)
    for i in range(1, m + 1):
        v = o + i * e
        cells[i, 0] = (NEG, NEG, v, 0, True) if v >= -X else (NEG, NEG, NEG, 0, False)
    windows = []
    best, best_i, best_j = 0, 0, 0
    slot = _Slot()
    lo_p, z_p, pf, Bst = 1, 0, 0, 0
    nchunks = (n + W - 1) // W
    for c in range(nchunks if m else 0):
        c0, c1 = c * W, min(n, (c + 1) * W)
        lo, Bs = 1, 0
        if c > 0 and not o + c0 * e >= -X:
            if pf == 0:
                break                                   # nothing enters the chunk: the pair ends
            lo = pf
            Bs = slot[pf - 1][2] if pf > lo_p else Bst
        cols = range(c0 + 1, c1 + 1)
        if lo == 1:
            Hp = {j: max(cells[0, j][:3]) for j in cols}
            hd = max(cells[0, c0][:3])                  # P(0, c0)
        else:
            Hp = {j: NEG for j in cols}
            hd = NEG
        Dn = {j: NEG for j in cols}
        Bp = {j: Bs for j in cols}
        cb, cb_i, cb_j = 0, 0, 0
        publish = c + 1 < nchunks
        new, live, last_B = {}, 0, Bs
        r = lo
        while r <= m:
            if c == 0:
                v = o + r * e
                inH, inF, inB = (v if v >= -X else NEG), NEG, 0
            elif r <= z_p:
                inH, inF, inB = slot[r]
            else:
                inH, inF, inB = NEG, NEG, 0
            F, Bl, alive = inF, inB, inH > _REAL
            S = sc.S[d[r - 1]]
            for j in cols:
                M = _plus(hd, int(S[q[j - 1]]))
                I, D = F, Dn[j]
                P3 = max(M, I, D)
                Bin = max(Bp[j], Bl)
                if P3 < Bin - X:
                    cells[r, j] = (NEG, NEG, NEG, Bin, False)
                    P, Bl, F, Dn[j] = NEG, Bin, NEG, NEG
                else:
                    Bl = max(Bin, P3)
                    cells[r, j] = (M, I, D, Bl, True)
                    P = P3
                    tO = _plus(M, o)
                    F, Dn[j] = _plus(max(tO, I), e), _plus(max(tO, D), e)
                    alive = True
                    if M > cb:                          # rows, then columns, rising
                        cb, cb_i, cb_j = M, r, j
                Bp[j] = Bl
                hd, Hp[j] = Hp[j], P
            hd = inH
            last_B = Bl
            if alive or (c > 0 and r <= z_p):
                live = r
            new[r] = (Hp[c1], F, Bl)
            if live != r:
                break                                   # the first row that is not alive
            r += 1
        z = min(m, max(live, lo))
        windows.append((lo, z))
        if cb > best or (cb == best and cb > 0 and cb_i < best_i):
            best, best_i, best_j = cb, cb_i, cb_j
        if publish:
            assert new[z][2] == last_B                  # B stands still below z
            slot = _Slot({r: v for r, v in new.items() if r <= z})
            live_rows = [r for r in range(lo, z + 1) if slot[r][0] > _REAL]
            pf = live_rows[0] if live_rows else 0
            lo_p, z_p, Bst = lo, z, Bs
    computed = np.zeros((m + 1, n + 1), bool)
    for i, j in cells:
        computed[i, j] = True
    return cells, computed, windows, (best, best_i, best_j)


def align(q: bytes, d: bytes, X: int, scoring=None, W: int = 1024, walk: bool = True):
    """(Alignment, alive, computed, windows, steps): the alignment from the
    cells the schedule evaluated (the walk is xdrop_model's and fails on a cell
    that was not), the mask of the unpruned ones among them, the mask of the
    evaluated cells, the chunks' windows, and steps_bound of them."""
    sc = _scoring(scoring)
    o, e = sc.o, sc.e
    q, d = bytes(q), bytes(d)
    n, m = len(q), len(d)
    cells, computed, windows, (best, end_i, end_j) = schedule(q, d, X, sc, W)
    alive = np.zeros((m + 1, n + 1), bool)
    for (i, j), cell in cells.items():
        alive[i, j] = cell[4]
    steps = steps_bound(windows)
    if best == 0:
        z = 0 if walk else -1
        return Alignment(0, z, 0, z, 0), alive, computed, windows, steps
    if not walk:
        return Alignment(best, -1, end_j, -1, end_i), alive, computed, windows, steps
    i, j, st, ops = end_i, end_j, 0, []                 # st: 0 M, 1 I, 2 D
    while True:
        assert cells[i, j][4], "the walk stands on a pruned cell"
        if st == 0:
            if i == 0 or j == 0:
                assert i == 0 and j == 0
                break
            ops.append("=" if q[j - 1] == d[i - 1] else "X")
            v = cells[i, j][0] - int(sc.S[d[i - 1]][q[j - 1]])
            i, j = i - 1, j - 1
            st = next(k for k in range(3) if cells[i, j][k] == v)
        else:
            ops.append("ID"[st - 1])
            cur = cells[i, j][st]
            i, j = (i, j - 1) if st == 1 else (i - 1, j)
            if not (cells[i, j][st] > _REAL and cells[i, j][st] + e == cur):
                assert cells[i, j][0] + o + e == cur
                st = 0
    cigar = []
    for op in reversed(ops):
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return Alignment(best, 0, end_j, 0, end_i, cigar), alive, computed, windows, steps
