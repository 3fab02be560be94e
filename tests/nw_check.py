"""Shared helpers for NW parity tests (imports the oracle: test-only)."""
from __future__ import annotations

import numpy as np

SCHEME = (5, -4, -8, -6)

# (match, mismatch, gap_open, gap_extend) -> the range guard whose edge the
# scheme sits on (DESIGN.md "Scoring-scheme domain")
SCHEMES = {
    (5, -4, -8, -6): "default",
    (2, -3, -5, -2): "small custom scheme",
    (1, 0, 0, 0): "pen = 2, every cell ties",
    (1, 0, -1, 0): "pen = 2, zero extend",
    (5, -4, 0, -6): "zero open: extend ties with open",
    (5, -4, -8, 0): "zero extend: no packed table",
    (8, -8, -16, -12): "pen = 32, rebase refused",
    (12, -4, -20, -16): "pen = 32, larger growth",
    (5, -12, -8, -6): "pen = 34: i32 only",
    (3, -13, -8, -6): "pen = 32, cmm < 0: packed without the table",
    (6, 2, -8, -6): "positive mismatch",
    (-1, -3, -4, -2): "negative match",
    (5, 5, -8, -6): "pen = 0",
    (4, 5, -8, -6): "pen < 0",
    (60, -4, -8, -6): "i32 pen_max = 256",
    (61, -4, -8, -6): "i32 pen_max = 260",
    (5, -4, -8, -20): "steep extend",
    (16, 0, -30, -40): "bonuses near a byte; i32 only (152 columns exceed its int16 range)",
    (5, -4, -6800, -1): "huge open: rebase frame only",
    (5, -4, -2000, -1): "pk_tab_ok accepts",
    (5, -4, -2001, -1): "pk_tab_ok refuses",
    (8, -8, -8, -7): "64-lane rebasing frame near its bound",
    (5, -4, -8, -600): "sentinel reached at 54 columns",
    (5, -4, 2, -6): "positive open",
}
SENTINEL_SCHEME = (5, -4, -8, -600)


def rand_seq(rng: np.random.Generator, n: int, alphabet: bytes = b"ACGT") -> bytes:
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def path_score(query: bytes, db: bytes, cigar, scheme=SCHEME) -> tuple[int, bool]:
    """Score of an alignment path under the reference recurrences (I/D open
    only from M, needleman_wunsch_affine.rs:87-94); second value is False if
    the path breaks a recurrence rule or does not consume both sequences."""
    mat, mis, go, ge = scheme
    i = j = 0
    state = "M"
    score = 0
    ok = True
    for n, op in cigar:
        for _ in range(n):
            if op in "=X":
                if j >= len(query) or i >= len(db):
                    return score, False
                eq = query[j] == db[i]
                if (op == "=") != eq:
                    ok = False
                score += mat if eq else mis
                i += 1; j += 1; state = "M"
            elif op == "I":
                if state == "D" or j >= len(query):
                    ok = False
                score += (go + ge) if state == "M" else ge
                j += 1; state = "I"
            else:
                if state == "I" or i >= len(db):
                    ok = False
                score += (go + ge) if state == "M" else ge
                i += 1; state = "D"
    return score, ok and i == len(db) and j == len(query)


def expand(cigar) -> str:
    return "".join(op * n for n, op in cigar)
