"""Pins tests/ends_free_model.py (the checker of the ends-free engine) against
brute-force enumeration written here, independent of the model: every
alignment of every substring pair, gaps opening from M only (an I run and a D
run are never adjacent); and its canonical choices against
tests/golden/ends_free_model_pins.json.  CPU only."""
import functools
import itertools
import json
import os
import random

import pytest

import ends_free_model as model

SCHEMES = [(5, -4, -8, -6), (1, -1, 0, -1), (2, -3, -5, -2)]
MODES = [model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP, model.EXTEND]


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
    if mode == model.OVERLAP:      # from row 0 or column 0 to row m or column n, or nothing at all
        n, m = len(q), len(d)
        return max([0] + [_best_global(q[a0:a1], d[b0:b1], scheme)
                          for a0 in range(n + 1) for a1 in range(a0, n + 1)
                          for b0 in range(m + 1) for b1 in range(b0, m + 1)
                          if (a0 == 0 or b0 == 0) and (a1 == n or b1 == m)])
    if mode == model.EXTEND:       # a prefix of d with a prefix of q, or nothing at all
        return max([0] + [_best_global(q[:j], d[:i], scheme)
                          for i in range(len(d) + 1) for j in range(len(q) + 1)])
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
    elif a.score == 0:
        assert a.cigar == [] and a.record() == (0, 0, 0, 0, 0, 0, 0, 0)
    elif mode == model.OVERLAP:
        assert a.q_begin == 0 or a.db_begin == 0
        assert a.q_end == len(q) or a.db_end == len(d)
    elif mode == model.EXTEND:
        assert (a.q_begin, a.db_begin) == (0, 0)
        assert a.cigar[-1][1] in "=X", "ending in a gap is never better"
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


# ------------------------------------------------------------------ the pins
def _pins():
    """(q, d, mode, scoring, record, CIGAR string) of every entry."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "ends_free_model_pins.json")) as f:
        for entry in json.load(f)["scorings"]:
            sc = entry["scoring"]
            sc = tuple(sc) if isinstance(sc, list) else model.matrix_scoring(
                sc["alphabet"].encode(), sc["table"], sc["o"], sc["e"])
            for mode in MODES:
                for (q, d), (record, cigar) in zip(entry["pairs"], entry["expected"][str(mode)]):
                    yield q.encode(), d.encode(), mode, sc, tuple(record), cigar


def test_pins():
    """The model gives the records and CIGARs the four models it replaced
    gave (the fixture was written from them), with and without the walk and
    with rolling rows; and the fixture holds the cases that make this a pin of
    the tie rules.  A CIGAR that starts with 'I' or 'D' is asked of every mode
    whose definition admits one: a local alignment starts with '=' or 'X',
    and semi-global's D(i,0) is -infinity, so those are asserted absent."""
    first = {mode: set() for mode in MODES}
    overlap_ties = local_ties = entries = 0
    for q, d, mode, sc, record, cigar in _pins():
        entries += 1
        a = model.align(q, d, mode, sc)
        assert (a.record(), "".join(f"{k}{op}" for k, op in a.cigar)) == (record, cigar), (q, d, mode)
        b = model.align(q, d, mode, sc, walk=False)
        ends = (a.score, -1, a.q_end, -1, a.db_end)
        if mode != model.SEMI_GLOBAL and a.score == 0:
            ends = (0, -1, 0, -1, 0)
        assert (b.score, b.q_begin, b.q_end, b.db_begin, b.db_end) == ends and b.cigar == []
        assert model.linear_ends(q, d, mode, sc) == (a.score, a.q_end, a.db_end), (q, d, mode)
        first[mode].add(cigar.lstrip("0123456789")[:1])       # "" for the empty alignment
        if mode == model.OVERLAP and a.score:
            info = model.end_info(q, d, sc)
            overlap_ties += len(info["col_ties"]) + len(info["row_ties"]) > 1
        if mode == model.LOCAL:
            local_ties += model.tied_ends(q, d, mode, sc)[0] > 1
    assert entries == 5 * 40 * 4
    assert "" in first[model.LOCAL] and not first[model.LOCAL] & {"I", "D"}
    assert "I" in first[model.SEMI_GLOBAL] and "D" not in first[model.SEMI_GLOBAL]
    assert first[model.OVERLAP] >= {"", "I", "D"} and first[model.EXTEND] >= {"", "I", "D"}
    assert overlap_ties >= 10 and local_ties >= 10
