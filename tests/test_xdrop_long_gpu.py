"""GPU: X-drop extension of pairs of any length, saln_ends_free_xdrop_long_*
(ef_xdrop_fill_long_kernel in ends_free_xdrop_long_kernels.hip): the chunked
fill with a window of rows per chunk, dead chunks skipped and the pair left at
the first of them.  Every comparison is exact against the plain model
(xdrop_model.py): the record, the CIGAR word for word, score only as well, and
`reserved` within the bound that the schedule model (xdrop_long_model.py)
derives from the chunks' windows.  The inputs' preconditions are asserted from
the models first, and without a device in test_the_cases_are_what_they_claim."""
import random

import pytest

import ends_free_model as efm
import test_extend_long_gpu as elg
import xdrop_long_model as lm
import xdrop_model as model
from test_extend_gpu import DEFAULT, anchored, rand_seq

EXTEND = efm.EXTEND
CHUNK = 1024
_cache = {}


def expect(q, d, X, name):
    """(Alignment, alive, L, windows) of the models, once per (pair, X, scoring)."""
    key = (q, d, X, name)
    if key not in _cache:
        msc = elg.scoring(None, name)[1]
        a, alive, L = model.align(q, d, X, msc)
        _cache[key] = (a, alive, L, lm.schedule(q, d, X, msc)[2])
    return _cache[key]


def bound(q, d, X, name):
    """The most steps `reserved` may report: the class fill's for a pair the
    class limits hold, else the chunked fill's from its windows."""
    a, alive, L, windows = expect(q, d, X, name)
    if not q:
        return 0
    if len(q) <= 1024 and len(d) <= 65000:
        lanes = next(g for g, k in ((16, 10), (16, 16), (64, 8), (64, 16)) if len(q) <= g * k)
        return model.steps_bound(len(d), L, lanes)
    return lm.steps_bound(windows)


def check(saln, qs, ds, pairs, X, name, cigar=True):
    """One batch under X, with words and score only, against the models."""
    sc = elg.scoring(saln, name)[0]
    sres, scig = saln.xdrop_extend_long_batch(qs, ds, pairs, xdrop=X, scoring=sc, cigar=False)
    res, cig = saln.xdrop_extend_long_batch(qs, ds, pairs, xdrop=X, scoring=sc) if cigar else (None, None)
    assert len(sres) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        q, d = qs[a], ds[b]
        want = expect(q, d, X, name)[0]
        tag = (k, len(q), len(d), X)
        ends = (want.score, 0, -1, want.q_end, -1, want.db_end, 0) if want.score else (0, 0, -1, 0, -1, 0, 0)
        steps, most = int(sres["reserved"][k]), bound(q, d, X, name)
        if len(pairs) < 100:
            print(tag, "steps", steps, "bound", most)
        assert tuple(int(v) for v in sres[k])[:7] == ends and scig[k] == [], tag
        assert (1 if q and d else 0) <= steps <= most, (tag, steps, most)
        if cigar:
            assert tuple(int(v) for v in res[k])[:7] == want.record()[:7], tag
            assert cig.words(k).tolist() == efm.cigar_words(want.cigar), tag
            assert saln.alignment_score(q, d, (res[k], cig[k]), sc) == want.score, tag
            assert int(res["reserved"][k]) == steps, tag      # the same fill, with and without codes
    return (res, cig) if cigar else (sres, scig)


def is_long(q, d):
    return len(q) > 1024 or len(d) > 65000


# ------------------------------------------------------------------ the pairs
def mutated(rng, w, rate=0.05, letters=b"ACGT"):
    out = bytearray(w)
    for k in range(8, len(w) - 8):
        if rng.random() < rate:
            out[k] = rng.choice(letters)
    return bytes(out)


def diagonal_pair():
    rng = random.Random(0xD1A6)
    q = rand_seq(rng, 1100, b"ACGT")
    return q, mutated(rng, q)


def dead_chunks_pair():
    rng = random.Random(0xDEAD)
    q = rand_seq(rng, 2100, b"ACGT")
    return q, mutated(rng, q[:400]) + rand_seq(rng, 300, b"ACGT")


def row0_pair():
    return elg.border_pairs()[1]


def crossing_pair(name):
    return elg.crossing_pairs(elg.scoring(None, name)[2])[1]


def deletion_pairs():
    return list(zip(elg.border_pairs()[0], (64, 65, 130)))


def tall_pair():
    rng = random.Random(0x65009)
    q = rand_seq(rng, 40, b"ACGT")
    return q, anchored(rng, q, 60, b"ACGT") + rand_seq(rng, 64941, b"ACGT")


ROW0_X = 2 + 1030                    # -(o + 1,030 e) under (5, -4, -2, -1)
CROSS_X = 2 + (2049 - 130)           # the insertion over the junk, o + 1,919 e, under gaps (-2, -1)
MIXED_X = CROSS_X


def mixed_pairs():
    """Five pairs of mixed fates under the cheap-gap scoring and MIXED_X: three
    chunks all run; random against random; a match that ends at (100, 100), whose
    insertion run dies at column 2,019, before chunk 2; a pair of the class path; a
    two-chunk diagonal.  Four dbs share the 128-255 rows bucket, so they share
    a launch."""
    rng = random.Random(0x51A7)
    a = rand_seq(rng, 100, b"ACGT")
    q4 = rand_seq(rng, 1030, b"ACGT")
    return [crossing_pair("cheap"),
            (rand_seq(rng, 2100, b"ACGT"), rand_seq(rng, 200, b"ACGT")),
            (a + b"N" * 2000, mutated(rng, a) + b"M" * 40),
            (rand_seq(rng, 500, b"ACGT"), rand_seq(rng, 120, b"ACGT")),
            (q4, mutated(rng, q4[:220]))]


def preconditions(key):
    if key == "diagonal":
        q, d = diagonal_pair()
        a, alive, L, windows = expect(q, d, 60, "default")
        first = min(i for i in range(len(d) + 1) if alive[i, CHUNK + 1:].any())
        assert first > 1000 and len(windows) == 2 and 1000 < windows[1][0] <= first
        assert a.score > 4000 and bound(q, d, 60, "default") < 0.7 * 2 * (1100 + 63)
    elif key == "dead":
        q, d = dead_chunks_pair()
        a, alive, L, windows = expect(q, d, 100, "default")
        assert not alive[:, CHUNK + 1:].any() and len(windows) == 1      # chunks 1 and 2 hold no live cell
        assert 392 <= a.q_end <= 440 and 392 <= a.db_end <= 440 and a.db_end < L < 700 and a.score > 1500
        assert windows == [(1, L)] and bound(q, d, 100, "default") == L + 64
    elif key == "row0":
        q, d = row0_pair()
        a = expect(q, d, ROW0_X, "row0")[0]
        assert a.cigar == [(1030, "I"), (300, "=")] and a.score == 468
        b, alive, L, windows = expect(q, d, ROW0_X - 1, "row0")
        assert alive[0, 1029] and not alive[0, 1030] and b.score < 468 and b.cigar[:1] != [(1030, "I")]
    elif key in ("cheap", "x24"):
        q, d = crossing_pair(key)
        msc = elg.scoring(None, key)[1]
        plain = efm.align(q, d, EXTEND, msc)
        a, alive, L, windows = expect(q, d, CROSS_X, key)
        assert a == plain and len(windows) == 3 and windows[2][0] > 1     # row 0 is pruned at column 2,048
        assert any(n == 1919 and op == "I" for n, op in a.cigar)
        b = expect(q, d, CROSS_X - 1, key)[0]
        assert 0 < b.score < a.score
    elif key.startswith("deletions"):
        for (q, d), g in deletion_pairs()[int(key[-1]):int(key[-1]) + 1]:
            X = 8 + 6 * g
            a = expect(q, d, X, "default")[0]
            assert a.cigar == [(g, "D"), (1100, "=")] and a.score == 5500 - X
            b, alive, L, windows = expect(q, d, X - 1, "default")
            assert alive[g - 1, 0] and not alive[g, 0] and b.score < a.score
    elif key == "tall":
        q, d = tall_pair()
        a, alive, L, windows = expect(q, d, 40, "default")
        assert a.score > 0 and L < 200 and bound(q, d, 40, "default") < 300
    elif key == "mixed":
        want = [expect(q, d, MIXED_X, "cheap") for q, d in mixed_pairs()]
        assert [len(w[3]) for w in want[:3]] == [3, 3, 2] and len(want[4][3]) == 2
        assert want[2][0].q_end == 100 and want[0][0].q_end == 2049
        assert [is_long(q, d) for q, d in mixed_pairs()] == [True, True, True, False, True]


KEYS = ("diagonal", "dead", "row0", "cheap", "x24", "deletions0", "deletions1", "deletions2", "tall", "mixed")


@pytest.mark.parametrize("key", KEYS)
def test_the_cases_are_what_they_claim(key):
    preconditions(key)


# ------------------------------------------------------------------ the cases
@pytest.mark.gpu
def test_diagonal_across_a_chunk_edge(saln):
    """Chunk 1 starts at the band, not at row 1."""
    preconditions("diagonal")
    q, d = diagonal_pair()
    assert saln.ends_free.pair_path_long(len(q), len(d)) == (1, 2)
    res, _ = check(saln, [q], [d], [(0, 0)], 60, "default")
    assert int(res["reserved"][0]) < 0.7 * 2 * (1100 + 63)


@pytest.mark.gpu
def test_dead_chunks_do_not_run(saln):
    """Steps within the bound of chunk 0 alone, and the class fill's record on
    the pair cut to its first 1,024 columns, which keeps every live cell."""
    preconditions("dead")
    q, d = dead_chunks_pair()
    res, cig = check(saln, [q], [d], [(0, 0)], 100, "default")
    cres, ccig = saln.ends_free_align_batch([q[:CHUNK]], [d], mode=EXTEND, xdrop=100)
    assert tuple(int(v) for v in cres[0])[:7] == tuple(int(v) for v in res[0])[:7]
    assert ccig.words(0).tolist() == cig.words(0).tolist()


@pytest.mark.gpu
def test_row_0_live_past_a_chunk_edge(saln):
    preconditions("row0")
    q, d = row0_pair()
    for X in (ROW0_X, ROW0_X - 1):
        check(saln, [q], [d], [(0, 0)], X, "row0")


@pytest.mark.gpu
@pytest.mark.parametrize("key", ("cheap", "x24"))
def test_insertion_across_the_edge_at_column_1024(saln, key):
    preconditions(key)
    q, d = crossing_pair(key)
    for X in (CROSS_X, CROSS_X - 1):
        check(saln, [q], [d], [(0, 0)], X, key)


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1, 2))
def test_column_0(saln, which):
    """A leading deletion of 64, 65 or 130 rows at X = its cost and one less."""
    preconditions("deletions%d" % which)
    (q, d), g = deletion_pairs()[which]
    for X in (8 + 6 * g, 8 + 6 * g - 1):
        check(saln, [q], [d], [(0, 0)], X, "default")


@pytest.mark.gpu
def test_db_above_the_class_limit_stops_early(saln):
    preconditions("tall")
    q, d = tall_pair()
    assert saln.ends_free.pair_path_long(40, 65001) == (1, 1)
    res, _ = check(saln, [q], [d], [(0, 0)], 40, "default", cigar=False)
    assert int(res["reserved"][0]) < 300 < 65001 + 63


@pytest.mark.gpu
def test_large_x_is_plain_extension_word_for_word(saln):
    for name, (q, d) in (("default", diagonal_pair()), ("cheap", crossing_pair("cheap"))):
        sc, msc, _ = elg.scoring(saln, name)
        X = model.no_drop(len(q), len(d), msc)
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=X, scoring=sc)
        pres, pcig = saln.ends_free_align_long_batch([q], [d], mode=EXTEND, scoring=sc)
        assert tuple(int(v) for v in res[0])[:7] == tuple(int(v) for v in pres[0])[:7] and int(res["score"][0]) > 0
        assert cig.words(0).tolist() == pcig.words(0).tolist()
        assert int(pres["reserved"][0]) == 0 < int(res["reserved"][0])


@pytest.mark.gpu
def test_three_chunks_and_a_slot_reused_by_pairs_of_mixed_fates(saln):
    """12,300 pairs over five distinct ones, more than three times the 4,096
    waves of a launch: every wave runs several pairs of different lengths and
    fates in its boundary slot one after the other (score only), then fifteen
    with words."""
    preconditions("mixed")
    five = mixed_pairs()
    qs, ds = [p[0] for p in five], [p[1] for p in five]
    rng = random.Random(0xA11)
    order = [rng.randrange(5) for _ in range(12300)]
    check(saln, qs, ds, [(k, k) for k in order], MIXED_X, "cheap", cigar=False)
    check(saln, qs, ds, [(k % 5, k % 5) for k in range(15)], MIXED_X, "cheap")


@pytest.mark.gpu
def test_direction_left(saln):
    q, d = row0_pair()
    r, c = saln.xdrop_extend_long(q, d, xdrop=ROW0_X, scoring=elg.ROW0)
    lr, lc = saln.xdrop_extend_long(q[::-1], d[::-1], xdrop=ROW0_X, scoring=elg.ROW0, direction="left")
    assert tuple(int(v) for v in r)[:6] == (468, 0, 0, 1330, 0, 300) and c == [(1030, "I"), (300, "=")]
    assert tuple(int(v) for v in lr)[:6] == (468, 0, 0, 1330, 0, 300) and lc == c[::-1]
    assert saln.xdrop_steps(lr) == saln.xdrop_steps(r) > 0


@pytest.mark.gpu
def test_match_mismatch_matrix_equals_the_scalar_engine(saln):
    q, d = diagonal_pair()
    sm = saln.SubstitutionMatrix(b"ACGT", [[5 if a == b else -4 for b in range(4)] for a in range(4)], -8, -6)
    res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, scoring=DEFAULT)
    mres, mcig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, scoring=sm)
    assert tuple(int(v) for v in mres[0]) == tuple(int(v) for v in res[0])
    assert mcig.words(0).tolist() == cig.words(0).tolist() and int(res["score"][0]) > 4000
