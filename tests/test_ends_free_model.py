"""Pins tests/ends_free_model.py (the checker of the ends-free engine) against
brute-force enumeration written here, independent of the model: every
alignment of every substring pair, gaps opening from M only (an I run and a D
run are never adjacent).  CPU only."""
import functools
import itertools
import random

import pytest

import ends_free_model as model

SCHEMES = [(5, -4, -8, -6), (1, -1, 0, -1), (2, -3, -5, -2)]
MODES = [model.LOCAL, model.SEMI_GLOBAL]


@functools.lru_cache(maxsize=None)
def _op_strings(la, lb):
    """Every alignment of a query of la bases with a db of lb bases as a
    string of M / I / D columns, without an I next to a D."""
    out = []

    def rec(i, j, ops):
        if i == la and j == lb:
            out.append("".join(ops))
            return
        last = ops[-1] if ops else ""
        if i < la and j < lb:
            rec(i + 1, j + 1, ops + ["M"])
        if i < la and last != "D":
            rec(i + 1, j, ops + ["I"])
        if j < lb and last != "I":
            rec(i, j + 1, ops + ["D"])

    rec(0, 0, [])
    return out


def _score_ops(ops, a, b, scheme):
    ma, mi, o, e = scheme
    i = j = 0
    total, prev = 0, ""
    for op in ops:
        if op == "M":
            total += ma if a[i] == b[j] else mi
            i += 1
            j += 1
        else:
            total += e + (o if op != prev else 0)
            if op == "I":
                i += 1
            else:
                j += 1
        prev = op
    return total


@functools.lru_cache(maxsize=None)
def _best_global(a, b, scheme):
    return max(_score_ops(ops, a, b, scheme) for ops in _op_strings(len(a), len(b)))


def brute(q, d, mode, scheme):
    if mode == model.LOCAL:
        best = 0
        for a0, a1 in itertools.combinations(range(len(q) + 1), 2):
            for b0, b1 in itertools.combinations(range(len(d) + 1), 2):
                best = max(best, _best_global(q[a0:a1], d[b0:b1], scheme))
        return best
    best = None
    for b0 in range(len(d) + 1):
        for b1 in range(b0, len(d) + 1):
            v = _best_global(q, d[b0:b1], scheme)
            best = v if best is None else max(best, v)
    return best


def check_alignment(q, d, mode, scheme, a):
    """The CIGAR re-scores to the score, respects the ranges and tells '='
    from 'X' truthfully."""
    ma, mi, o, e = scheme
    assert 0 <= a.q_begin <= a.q_end <= len(q) and 0 <= a.db_begin <= a.db_end <= len(d)
    if mode == model.SEMI_GLOBAL:
        assert (a.q_begin, a.q_end) == (0, len(q))
    j, i = a.q_begin, a.db_begin
    total, prev = 0, None
    for n, op in a.cigar:
        assert n > 0 and op != prev, "runs are merged"
        assert not (prev in ("I", "D") and op in ("I", "D")), "an I run next to a D run"
        for _ in range(n):
            if op in "=X":
                assert (q[j] == d[i]) == (op == "="), (i, j, op)
                total += ma if op == "=" else mi
                i += 1
                j += 1
            elif op == "I":
                total += e
                j += 1
            else:
                total += e
                i += 1
        if op in "ID":
            total += o
        prev = op
    assert (j, i) == (a.q_end, a.db_end)
    assert total == a.score
    if mode == model.LOCAL:
        if a.score == 0:
            assert a.cigar == [] and a.record()[2:6] == (0, 0, 0, 0)
        else:
            assert a.cigar[0][1] in "=X" and a.cigar[-1][1] in "=X"


def _all_strings(alphabet, max_len):
    for n in range(max_len + 1):
        for t in itertools.product(alphabet, repeat=n):
            yield "".join(t).encode()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("mode", MODES)
def test_every_small_pair_over_ac(mode, scheme):
    strings = list(_all_strings("AC", 4))
    for q in strings:
        for d in strings:
            a = model.align(q, d, mode, scheme)
            assert a.score == brute(q, d, mode, scheme), (q, d)
            check_alignment(q, d, mode, scheme, a)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("mode", MODES)
def test_random_pairs_over_acgt(mode, scheme):
    rng = random.Random(0xE0F + 7 * mode + scheme[0])
    for _ in range(250):
        q = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 5))).encode()
        d = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 6))).encode()
        a = model.align(q, d, mode, scheme)
        assert a.score == brute(q, d, mode, scheme), (q, d)
        check_alignment(q, d, mode, scheme, a)


def test_score_only_matches_walk():
    rng = random.Random(5)
    for mode in MODES:
        for _ in range(50):
            q = "".join(rng.choice("AC") for _ in range(rng.randint(0, 12))).encode()
            d = "".join(rng.choice("AC") for _ in range(rng.randint(0, 12))).encode()
            a, b = model.align(q, d, mode), model.align(q, d, mode, walk=False)
            assert (a.score, a.q_end, a.db_end) == (b.score, b.q_end, b.db_end)
            assert (b.q_begin, b.db_begin, b.cigar) == (-1, -1, [])


def test_tie_rules():
    # the same window twice: the smallest row wins
    a = model.align(b"ACGT", b"ACGTTTTTACGT", model.SEMI_GLOBAL)
    assert (a.score, a.db_begin, a.db_end, a.cigar) == (20, 0, 4, [(4, "=")])
    a = model.align(b"ACGT", b"ACGTTTTTACGT", model.LOCAL)
    assert (a.score, a.db_end, a.q_end) == (20, 4, 4)
    # the same row twice: the smallest column wins
    a = model.align(b"ACGTCCACGT", b"ACGT", model.LOCAL)
    assert (a.score, a.q_begin, a.q_end, a.db_begin, a.db_end) == (20, 0, 4, 0, 4)
    assert model.tied_ends(b"ACGT", b"ACGTTTTTACGT", model.LOCAL) == (2, 2)
    assert model.tied_ends(b"ACGTCCACGT", b"ACGT", model.LOCAL) == (2, 1)


def test_empty_sides():
    for sc in SCHEMES:
        o, e = sc[2], sc[3]
        a = model.align(b"", b"ACG", model.SEMI_GLOBAL, sc)
        assert a.record() == (0, 0, 0, 0, 0, 0, 0, 0)
        a = model.align(b"ACG", b"", model.SEMI_GLOBAL, sc)
        assert (a.score, a.cigar, a.db_begin, a.db_end) == (o + 3 * e, [(3, "I")], 0, 0)
        for q, d in ((b"", b""), (b"", b"A"), (b"A", b"")):
            assert model.align(q, d, model.LOCAL, sc).record() == (0, 0, 0, 0, 0, 0, 0, 0)


def test_a_long_pair_is_quick():
    import time
    rng = random.Random(1)
    q = bytes(rng.choice(b"ACGT") for _ in range(1024))
    d = bytes(rng.choice(b"ACGT") for _ in range(300))
    t = time.perf_counter()
    for mode in MODES:
        check_alignment(q, d, mode, model.DEFAULT_SCORING, model.align(q, d, mode))
    assert time.perf_counter() - t < 5.0
