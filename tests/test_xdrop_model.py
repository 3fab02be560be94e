"""Holds tests/xdrop_model.py (the checker of the X-drop extension,
saln_ends_free_xdrop_*) to ends_free_model's EXTEND at large X, to other
evaluation orders, to monotonicity in X, to its own words and path, and to
hand-derived cases on the strict boundary.  CPU only."""
import itertools
import random

import pytest

import ends_free_model as efm
import xdrop_model as model
from test_extend_gpu import ALPHABET24, GAPS24, TABLE24, anchored, rand_seq
from test_extend_model import check_alignment

DEFAULT = (5, -4, -8, -6)
OPEN0 = (5, -4, 0, -3)
XS = (0, 3, 9, 20, 45, 10 ** 6)


def scorings():
    return [efm.scalar_scoring(*DEFAULT), efm.scalar_scoring(*OPEN0),
            efm.matrix_scoring(ALPHABET24, TABLE24, *GAPS24)]


def random_pairs(count, seed, hi=28):
    rng = random.Random(seed)
    for k in range(count):
        letters = b"ACGT" if k % 3 else ALPHABET24
        q = rand_seq(rng, rng.randint(0, hi), letters)
        yield q, anchored(rng, q, rng.randint(0, hi), letters)


def same_as_extend(q, d, sc):
    X = model.no_drop(len(q), len(d), sc)
    for walk in (True, False):
        want = efm.align(q, d, efm.EXTEND, sc, walk=walk)
        got, alive, L = model.align(q, d, X, sc, walk=walk)
        assert got == want, (q, d)
    assert alive.all() and L == len(d)


def test_large_x_is_extend_on_every_small_pair():
    sc = efm.scalar_scoring(*DEFAULT)
    seqs = [bytes(s) for n in range(5) for s in itertools.product(b"AC", repeat=n)]
    for q in seqs:
        for d in seqs:
            same_as_extend(q, d, sc)


def test_large_x_is_extend_on_random_pairs():
    for sc in scorings():
        for q, d in random_pairs(60, 0x1A26E):
            same_as_extend(q, d, sc)


def in_order(q, d, X, sc, order):
    """The tables by xdrop_model.cell with the cells visited in `order`."""
    t = {(0, 0): model.ORIGIN}
    for i, j in order:
        if (i, j) == (0, 0):
            continue
        up, left = t.get((i - 1, j)), t.get((i, j - 1))
        assert (up is not None) == (i > 0) and (left is not None) == (j > 0), "not a valid schedule"
        if i and j:
            dg = t[i - 1, j - 1]
            t[i, j] = model.cell(max(dg[:3]), up, left, int(sc.S[d[i - 1]][q[j - 1]]), sc.o, sc.e, X)
        else:
            t[i, j] = model.cell(efm.NEG, up, left, None, sc.o, sc.e, X)
    return t


def test_the_order_of_evaluation_does_not_matter():
    """Row-major (the model), column-major and anti-diagonal order give the
    same tables, and the rows the model skips after a row without an unpruned
    cell hold none."""
    for sc in scorings():
        for k, (q, d) in enumerate(random_pairs(50, 0x02DE2, hi=22)):
            n, m = len(q), len(d)
            cells = [(i, j) for i in range(m + 1) for j in range(n + 1)]
            for X in XS:
                rows = model.fill(q, d, X, sc, stop=False)
                want = {(i, j): rows[i][j] for i, j in cells}
                assert in_order(q, d, X, sc, sorted(cells, key=lambda c: (c[1], c[0]))) == want
                assert in_order(q, d, X, sc, sorted(cells, key=lambda c: (c[0] + c[1], c[0]))) == want
                early = model.fill(q, d, X, sc)
                assert early == rows[:len(early)]
                assert not any(c[4] for row in rows[len(early):] for c in row)
                a, alive, L = model.align(q, d, X, sc)
                assert model.align(q, d, X, sc, stop=False)[0] == a
                assert L == max(i for i, j in cells if want[i, j][4]) and alive[0, 0]


def test_the_score_is_monotone_in_x_and_never_above_extend():
    for sc in scorings():
        for q, d in random_pairs(60, 0x3070):
            scores = [model.align(q, d, X, sc, walk=False)[0].score for X in XS]
            assert scores == sorted(scores), (q, d, scores)
            assert scores[-1] == efm.align(q, d, efm.EXTEND, sc, walk=False).score
            assert scores[0] >= 0


def test_the_words_rescore_and_the_path_never_drops_more_than_x():
    seen = 0
    for sc in scorings():
        for q, d in random_pairs(60, 0x9A78, hi=40):
            for X in XS:
                path = []
                a, alive, L = model.align(q, d, X, sc, path=path)
                check_alignment(q, d, sc, a)
                assert a.db_end <= L <= len(d)
                if not a.score:
                    continue
                rows = model.fill(q, d, X, sc)
                best = 0
                for i, j in reversed(path):       # from the origin to the end cell
                    assert alive[i, j]
                    P = max(rows[i][j][:3])
                    assert P >= best - X, (q, d, X, i, j)
                    best = max(best, P)
                assert path[-1] == (0, 0) and path[0] == (a.db_end, a.q_end)
                seen += 1
    assert seen > 300


# ---------------------------------------------------------------- the strict boundary, by hand
S1 = rand_seq(random.Random(0xB10C1), 30, b"ACGT")
S2 = rand_seq(random.Random(0xB10C2), 30, b"ACGT")


def junk_pair(g):
    """Two blocks of 30 matches around g mismatched columns ('N' on 'M')."""
    return S1 + b"N" * g + S2, S1 + b"M" * g + S2


@pytest.mark.parametrize("g", (1, 5, 12))
def test_a_junk_stretch_of_exactly_x_survives(g):
    """After the first block P = 150 = B; the g mismatches take P down to
    150 - 4 g at the junk's last column, the lowest point of the path, and every
    way around the junk costs more.  4 g <= X keeps the path; X = 4 g - 1, under
    which the stretch costs X + 1, prunes its last cell."""
    q, d = junk_pair(g)
    a, alive, L = model.align(q, d, 4 * g)
    assert (a.score, a.q_end, a.db_end) == (300 - 4 * g, 60 + g, 60 + g)
    assert a.cigar == [(30, "="), (g, "X"), (30, "=")] and L == 60 + g
    assert alive[30 + g, 30 + g]
    a, alive, L = model.align(q, d, 4 * g - 1)
    assert (a.score, a.q_end, a.db_end) == (150, 30, 30) and a.cigar == [(30, "=")]
    assert not alive[30 + g, 30 + g] and alive[30 + g - 1, 30 + g - 1]    # 4 (g - 1) <= X still
    assert L < 60 + g
    assert efm.align(q, d, efm.EXTEND).score == 300 - 4 * g


@pytest.mark.parametrize("k", (1, 7, 100))
def test_row_0_and_column_0_by_their_closed_forms(k):
    """(0, j) is unpruned iff o + j e >= -X, (i, 0) likewise: a leading
    insertion (deletion) of k survives X = 8 + 6 k and not one less."""
    s = rand_seq(random.Random(0xC0), 160, b"ACGT")
    X = 8 + 6 * k
    for q, d, lead in ((b"N" * k + s, s, "I"), (s, b"N" * k + s, "D")):
        a, alive, L = model.align(q, d, X)
        assert a.cigar == [(k, lead), (160, "=")] and a.score == 800 - X
        edge = alive[0] if lead == "I" else alive[:, 0]
        assert edge[:k + 1].all() and not edge[k + 1:].any()
        a, alive, L = model.align(q, d, X - 1)
        edge = alive[0] if lead == "I" else alive[:, 0]
        assert edge[:k].all() and not edge[k:].any()
        assert a.score < 800 - X and a.cigar[:1] != [(k, lead)]


def test_x_0_keeps_only_what_never_drops():
    a, alive, L = model.align(b"ACGTACGT", b"ACGTTCGT", 0)
    assert (a.score, a.cigar, L) == (20, [(4, "=")], 4)
    assert alive.sum() == 5                     # the diagonal's five cells
    a, alive, L = model.align(b"", b"ACG", 7)
    assert a.record() == (0, 0, 0, 0, 0, 0, 0, 0) and L == 0 and alive.tolist() == [[True]] + [[False]] * 3
    assert model.align(b"ACG", b"", 14)[1].tolist() == [[True, True, False, False]]
    assert model.steps_bound(5000, 120, 64) == 184 and model.steps_bound(90, 200, 16) == 106
