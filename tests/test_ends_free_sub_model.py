"""Pins tests/ends_free_model.py under a substitution matrix (the checker of
saln_ends_free_sub_*) against brute-force enumeration written here,
independent of the model, and its scalar scoring against the equivalent
match / mismatch matrix.  CPU only."""
import functools
import itertools
import random

import pytest

import ends_free_model as model

MODES = [model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP]

# Three symbols; rows: the db symbol, columns: the query symbol.  Asymmetric
# ([A][G] = 2, [G][A] = -4), a zero entry ([C][G]), a negative diagonal entry
# ([G][G]) and a positive off-diagonal entry ([A][G]).
ALPHABET3 = b"ACG"
TABLE3 = [[4, -3, 2],
          [-2, 3, 0],
          [-4, -5, -1]]
GAPS3 = [(-3, -1), (0, -2), (-6, -2)]


def _scoring3(gaps):
    return model.matrix_scoring(ALPHABET3, TABLE3, gaps[0], gaps[1])


def test_the_matrix_is_what_the_tests_need():
    t = TABLE3
    assert any(t[a][b] != t[b][a] for a in range(3) for b in range(3))
    assert any(v == 0 for r in t for v in r)
    assert any(t[a][a] < 0 for a in range(3))
    assert any(t[a][b] > 0 for a in range(3) for b in range(3) if a != b)
    sc = _scoring3(GAPS3[0])
    assert sc.S[ord("A")][ord("G")] == 2 and sc.S[ord("G")][ord("A")] == -4   # S[db][query]
    assert sc.S[ord("T")][ord("A")] == -5 and sc.S[ord("A")][ord("T")] == -5  # unknown: the smallest


# ------------------------------------------------------------------ brute force
@functools.lru_cache(maxsize=None)
def _op_strings(la, lb):
    """Every alignment of a query of la bytes with a db of lb bytes as a string
    of M / I / D columns, without an I next to a D."""
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


def _score_ops(ops, a, b, S, o, e):
    """a: the query bytes, b: the db bytes."""
    i = j = 0
    total, prev = 0, ""
    for op in ops:
        if op == "M":
            total += int(S[b[j]][a[i]])
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


def _best_global(a, b, sc, cache):
    key = (a, b)
    if key not in cache:
        cache[key] = max(_score_ops(ops, a, b, sc.S, sc.o, sc.e) for ops in _op_strings(len(a), len(b)))
    return cache[key]


def brute(q, d, mode, sc, cache):
    n, m = len(q), len(d)
    if mode == model.LOCAL:
        best = 0
        for a0, a1 in itertools.combinations(range(n + 1), 2):
            for b0, b1 in itertools.combinations(range(m + 1), 2):
                best = max(best, _best_global(q[a0:a1], d[b0:b1], sc, cache))
        return best
    if mode == model.SEMI_GLOBAL:
        return max(_best_global(q, d[b0:b1], sc, cache)
                   for b0 in range(m + 1) for b1 in range(b0, m + 1))
    # overlap: from row 0 or column 0 to row m or column n, or nothing at all
    best = 0
    for a0 in range(n + 1):
        for a1 in range(a0, n + 1):
            for b0 in range(m + 1):
                for b1 in range(b0, m + 1):
                    if (a0 == 0 or b0 == 0) and (a1 == n or b1 == m):
                        best = max(best, _best_global(q[a0:a1], d[b0:b1], sc, cache))
    return best


def check_alignment(q, d, mode, sc, a):
    """The CIGAR re-scores to the score under S[db][query], respects the
    ranges and tells '=' from 'X' by the bytes."""
    n, m = len(q), len(d)
    assert 0 <= a.q_begin <= a.q_end <= n and 0 <= a.db_begin <= a.db_end <= m
    if mode == model.SEMI_GLOBAL:
        assert (a.q_begin, a.q_end) == (0, n)
    elif a.score == 0:
        assert a.record() == (0, 0, 0, 0, 0, 0, 0, 0)
        return
    if mode == model.OVERLAP:
        assert a.q_begin == 0 or a.db_begin == 0
        assert a.q_end == n or a.db_end == m
    j, i = a.q_begin, a.db_begin
    total, prev = 0, None
    for k, op in a.cigar:
        assert k > 0 and op != prev, "runs are merged"
        assert not (prev in ("I", "D") and op in ("I", "D")), "an I run next to a D run"
        for _ in range(k):
            if op in "=X":
                assert (q[j] == d[i]) == (op == "="), (i, j, op)
                total += int(sc.S[d[i]][q[j]])
                i += 1
                j += 1
            elif op == "I":
                total += sc.e
                j += 1
            else:
                total += sc.e
                i += 1
        if op in "ID":
            total += sc.o
        prev = op
    assert (j, i) == (a.q_end, a.db_end)
    assert total == a.score
    if mode == model.LOCAL:
        assert a.cigar[0][1] in "=X" and a.cigar[-1][1] in "=X"


def _check_pair(q, d, mode, sc, cache):
    a = model.align(q, d, mode, sc)
    assert a.score == brute(q, d, mode, sc, cache), (q, d, mode)
    check_alignment(q, d, mode, sc, a)
    b = model.align(q, d, mode, sc, walk=False)
    if mode == model.SEMI_GLOBAL or a.score:
        assert (b.score, b.q_begin, b.q_end, b.db_begin, b.db_end) == (a.score, -1, a.q_end, -1, a.db_end)
    else:
        assert (b.score, b.q_begin, b.q_end, b.db_begin, b.db_end) == (0, -1, 0, -1, 0)
    assert b.cigar == []
    assert model.linear_ends(q, d, mode, sc) == (a.score, a.q_end, a.db_end), (q, d, mode)


@pytest.mark.parametrize("gaps", GAPS3)
@pytest.mark.parametrize("mode", MODES)
def test_every_small_pair_over_three_symbols(mode, gaps):
    sc, cache = _scoring3(gaps), {}
    strings = [bytes(t) for k in range(4) for t in itertools.product(ALPHABET3, repeat=k)]
    assert len(strings) == 40
    for q in strings:
        for d in strings:
            _check_pair(q, d, mode, sc, cache)


@pytest.mark.parametrize("mode", MODES)
def test_random_pairs_with_an_unknown_byte(mode):
    rng = random.Random(0x5B + mode)
    for gaps in GAPS3:
        sc, cache = _scoring3(gaps), {}
        for _ in range(120):
            q = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 5)))
            d = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 6)))
            _check_pair(q, d, mode, sc, cache)


def test_a_transposed_lookup_would_show():
    sc = _scoring3(GAPS3[0])
    # db A against query G scores 2, db G against query A scores -4
    assert model.align(b"G", b"A", model.LOCAL, sc).score == 2
    assert model.align(b"A", b"G", model.LOCAL, sc).score == 0
    a = model.align(b"G", b"A", model.LOCAL, sc)
    assert a.cigar == [(1, "X")]                       # positive, and still 'X': the bytes differ
    assert model.align(b"G", b"G", model.SEMI_GLOBAL, sc).cigar == [(1, "=")]   # '=' scoring -1
    assert model.align(b"G", b"G", model.SEMI_GLOBAL, sc).score == -1


# ------------------------------------------------------------------ the scalar schemes
SCHEMES = [(5, -4, -8, -6), (1, -1, 0, -1), (2, -3, -5, -2)]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_scalar_scoring_equals_the_match_mismatch_matrix(scheme):
    ma, mi, o, e = scheme
    table = [[ma if a == b else mi for b in range(4)] for a in range(4)]
    scalar, matrix = model.scalar_scoring(*scheme), model.matrix_scoring(b"ACGT", table, o, e)
    rng = random.Random(0xACE + ma)
    for k in range(150):
        q = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 40)))
        d = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 60)))
        if k % 3 == 0 and len(q) > 8:      # a planted overlap: a query suffix on a db prefix
            d = q[-8:] + d
        for mode in MODES + [model.EXTEND]:
            for walk in (True, False):
                a, b, c = (model.align(q, d, mode, sc, walk=walk) for sc in (scheme, scalar, matrix))
                assert a.record() == b.record() == c.record() and a.cigar == b.cigar == c.cigar, (q, d, mode)
            assert model.linear_ends(q, d, mode, scalar) == model.linear_ends(q, d, mode, matrix)


def test_case_insensitive_and_unknown():
    sc = model.matrix_scoring(b"AC", [[3, -2], [-1, 2]], -2, -1, unknown=-7, case_insensitive=True)
    assert sc.S[ord("a")][ord("C")] == -2 and sc.S[ord("c")][ord("a")] == -1
    assert sc.S[ord("N")][ord("A")] == -7 and sc.S[ord("A")][ord("N")] == -7
    a = model.align(b"aC", b"Ac", model.LOCAL, sc)
    assert (a.score, a.cigar) == (5, [(2, "X")])      # the symbols match, the bytes do not
