"""GPU: the X-drop extension, saln_ends_free_xdrop_* (ef_xdrop_fill_kernel in
ends_free_kernels.hip): extension alignment with cells pruned once they lie
more than X below the best unpruned value above and left of them, and the
fill's early stop.  Every comparison is exact against the plain model
(xdrop_model.py): the record, the CIGAR word for word, and `reserved` (the
steps the pair's group ran) within its bound, with CIGAR, score only and
through EndsFreePlan."""
import random

import numpy as np
import pytest

import ends_free_model as efm
import xdrop_model as model
from test_extend_gpu import DEFAULT, OPEN0, SCORINGS, anchored, rand_seq, scoring

EXTEND = efm.EXTEND
LARGE = 1 << 24          # far above 2 (n + m + 2) max|parameter| of every pair here

_expected = {}


def expect(q, d, X, name, msc):
    """(Alignment, L) of the model, once per (pair, X, scoring)."""
    key = (q, d, X, name)
    if key not in _expected:
        a, _, L = model.align(q, d, X, msc)
        _expected[key] = (a, L)
    return _expected[key]


def plan_results(saln, qs, ds, pairs, sc, X):
    import torch
    from sequencealigning_amd import _lib
    qb, qo = saln.pack_csr(qs)
    db, do = saln.pack_csr(ds)
    plan = saln.EndsFreePlan(qo, do, pairs, mode=EXTEND, scoring=sc, xdrop=X)
    dq = torch.from_numpy(np.concatenate([qb, np.zeros(16, np.uint8)])).cuda()
    dd = torch.from_numpy(np.concatenate([db, np.zeros(16, np.uint8)])).cuda()
    out = torch.full((plan.n_pairs * 8,), 77, dtype=torch.int32, device="cuda")
    plan.execute(dq, dd, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE)
    plan.close()
    return got


def check(saln, qs, ds, pairs, X, name, sc, msc):
    """One batch under X in the three forms against the model: record, words,
    and the steps within min(m, L) + lanes - 1 + 1 (the group votes after every
    step) and no fewer than L."""
    res, cig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, xdrop=X)
    sres, scig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, xdrop=X, cigar=False)
    pres = plan_results(saln, qs, ds, pairs, sc, X)
    assert len(res) == len(cig) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        q, d = qs[a], ds[b]
        want, L = expect(q, d, X, name, msc)
        tag = (k, len(q), len(d), X, q[:30], d[:30])
        assert tuple(int(v) for v in res[k])[:7] == want.record()[:7], tag
        assert cig.words(k).tolist() == efm.cigar_words(want.cigar), tag
        assert saln.alignment_score(q, d, (res[k], cig[k]), sc) == want.score, tag
        ends = (want.score, 0, -1, want.q_end, -1, want.db_end, 0) if want.score else (0, 0, -1, 0, -1, 0, 0)
        assert tuple(int(v) for v in sres[k])[:7] == ends and scig[k] == [], tag
        steps = int(res["reserved"][k])
        if q:
            lanes = saln.ends_free.pair_geometry(len(q))[0]
            assert max(L, 1) <= steps <= model.steps_bound(len(d), L, lanes), (tag, steps, L, lanes)
        else:
            assert steps == 0, tag
    assert (saln.xdrop_steps(sres) == res["reserved"]).all()      # the same fill, with and without codes
    assert (pres == sres).all()
    return res, cig


# ------------------------------------------------------------------ 1. class edges
EDGE_QUERIES = (1, 9, 10, 11, 160, 161, 256, 257, 512, 513, 1024)
EDGE_DBS = (1, 2, 15, 16, 17, 63, 64, 65, 90)
EDGE_XS = (0, 10, 40, LARGE)


def edge_batches(letters, seed):
    """Every class with pad columns (9, 11, 161, 257, 513) and full last lanes;
    each query against four dbs of 1 to 90 rows (mutated copies of its prefix
    plus a random tail), one per X, lengths and X rotating over the queries;
    and the empty sequences under every X."""
    rng = random.Random(seed)
    qs = [rand_seq(rng, n, letters) for n in EDGE_QUERIES] + [b""]
    ds, by_x = [b""], {X: [] for X in EDGE_XS}
    for a, q in enumerate(qs[:-1]):
        for k, X in enumerate(EDGE_XS):
            by_x[X].append((a, len(ds)))
            ds.append(anchored(rng, q, EDGE_DBS[(2 * a + 5 * k) % len(EDGE_DBS)], letters))
    for X in EDGE_XS:
        by_x[X] += [(len(qs) - 1, 1), (0, 0), (len(qs) - 1, 0), (4, 0)]    # n = 0, m = 0
    return qs, ds, by_x


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_class_edges(saln, name):
    sc, msc, letters = scoring(saln, name)
    qs, ds, by_x = edge_batches(letters, 0xD209)
    assert {saln.ends_free.pair_geometry(len(q)) for q in qs if q} == {(16, 10), (16, 16), (64, 8), (64, 16)}
    assert {len(ds[b]) for X in EDGE_XS for _, b in by_x[X]} >= set(EDGE_DBS)
    scores = {}
    for X in EDGE_XS:
        res, cig = check(saln, qs, ds, by_x[X], X, name, sc, msc)
        scores[X] = res["score"]
        for k in range(len(by_x[X]) - 4, len(by_x[X])):
            assert tuple(int(v) for v in res[k])[:7] == (0, 0, 0, 0, 0, 0, 0) and cig[k] == []
    assert (scores[LARGE] > 0).sum() >= 8 and (scores[40] > 0).sum() >= 5


# ------------------------------------------------------------------ 2. two blocks around a junk stretch
def junk_pair(letters, g, block=60):
    """Two homologous blocks around g columns of junk: the query's junk is one
    byte, the db's another, neither in the blocks."""
    rng = random.Random(0x70B + g)
    body = bytes(b for b in letters if b not in letters[-2:])
    s1, s2 = rand_seq(rng, block, body), rand_seq(rng, block, body)
    return s1 + letters[-1:] * g + s2, s1 + letters[-2:-1] * g + s2


def least_x_of_the_full_score(q, d, msc):
    """The smallest X under which the model scores what plain extension does
    (the score is monotone in X): the junk's cost."""
    full = efm.align(q, d, EXTEND, msc, walk=False).score
    lo, hi = 0, model.no_drop(len(q), len(d), msc)
    while lo < hi:
        mid = (lo + hi) // 2
        if model.align(q, d, mid, msc, walk=False)[0].score == full:
            hi = mid
        else:
            lo = mid + 1
    return lo, full


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_two_blocks_around_junk(saln, name):
    sc, msc, letters = scoring(saln, name)
    g = 6
    q, d = junk_pair(letters if name == "m24" else b"ACGTNM", g)
    cost, full = least_x_of_the_full_score(q, d, msc)
    if name != "m24":
        assert cost == 4 * g and full == 600 - 4 * g        # g mismatches, by hand
    assert cost > 1
    plain, _ = saln.ends_free_align_batch([q], [d], mode=EXTEND, scoring=sc)
    assert int(plain["score"][0]) == full
    for X, same in ((cost // 2, False), (cost - 1, False), (cost, True), (cost + 1, True), (3 * cost, True)):
        res, _ = check(saln, [q], [d], [(0, 0)], X, name, sc, msc)
        assert (int(res["score"][0]) == full) == same, (X, cost)
        assert 0 < int(res["score"][0]) <= full


# ------------------------------------------------------------------ 3. the early stop
def tail(rng, n, name, letters):
    """n db bytes no extension survives.  Default scheme: random bases.  With
    gap_open = 0 and under the matrix (random entries that average above 0)
    random sequences keep scoring upwards, so there it is one byte outside the
    queries' letters: a mismatch, or the matrix's smallest entry, against
    everything."""
    return rand_seq(rng, n, letters) if name == "default" else (b"O" if name == "m24" else b"N") * n


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
@pytest.mark.parametrize("n, m, hom", [(200, 5000, 100), (40, 65000, 40)])
def test_early_stop(saln, name, n, m, hom):
    """Homology in the first rows only: the fill leaves the pair soon after
    them, far before the m + lanes - 1 steps of the plain fill."""
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0xEA21 + n)
    body = letters[:-1] if name == "m24" else letters
    q = rand_seq(rng, n, body)
    d = anchored(rng, q, hom, body) + tail(rng, m - hom, name, body)
    X = 60
    res, _ = check(saln, [q], [d], [(0, 0)], X, name, sc, msc)
    L = expect(q, d, X, name, msc)[1]
    lanes = saln.ends_free.pair_geometry(n)[0]
    assert L < 4 * hom
    assert int(res["reserved"][0]) <= L + lanes - 1 + 1 < (m + lanes - 1) // 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_pad_lanes_stop_early(saln, name):
    """11 and 513 columns: lanes that hold nothing but pad columns (14 of 16,
    31 of 64) must not keep the group running."""
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0x9AD5)
    body = letters[:-1] if name == "m24" else letters
    qs = [rand_seq(rng, 11, body), rand_seq(rng, 513, body)]
    ds = [anchored(rng, q, 50, body) + tail(rng, 2950, name, body) for q in qs]
    res, _ = check(saln, qs, ds, [(0, 0), (1, 1)], 40, name, sc, msc)
    assert int(res["reserved"][0]) < 200 and int(res["reserved"][1]) < 300


# ------------------------------------------------------------------ 4. the vote of a group of 16
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_groups_of_16_vote_for_themselves(saln, name):
    """Twelve pairs of class 16 x 10 with dbs of one length: one launch, four
    pairs to a wave.  Pair 0 dies in its first rows, pair 1 runs every row,
    the others have homology of different lengths: no group stops because its
    neighbours are dead or runs on because they are alive."""
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0x16F0)
    body = letters[:-1] if name == "m24" else letters
    m = 150
    qs, ds = [], []
    for hom in (0, m, 20, 125, 60, 140, 5, 100, 35, 80, 110, 50):
        qs.append(rand_seq(rng, rng.randint(150, 160), body))
        ds.append(qs[-1][:hom] + tail(rng, m - hom, name, body))     # hom == m: matches to the last row
    assert {saln.ends_free.pair_geometry(len(q)) for q in qs} == {(16, 10)}
    pairs = [(k, k) for k in range(len(qs))]
    X = 30
    res, _ = check(saln, qs, ds, pairs, X, name, sc, msc)
    Ls = [expect(qs[k], ds[k], X, name, msc)[1] for k in range(len(qs))]
    assert Ls[0] < 40 and Ls[1] == m and len(set(Ls)) >= 8
    steps = [int(v) for v in res["reserved"]]
    assert steps[0] <= Ls[0] + 16 and steps[1] >= m and len(set(steps)) >= 8


# ------------------------------------------------------------------ 5. the borders
CHEAP_GAPS = [(5, -4, -2, -1), (5, -4, 0, -2)]      # a 100-column gap costs less than 60 matches earn


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", CHEAP_GAPS)
def test_lanes_that_have_not_started(saln, scheme):
    """160 columns whose path begins with a 100-column insertion: row 0 is
    unpruned up to column 100 iff X >= -(o + 100 e).  One short, lanes 0 to 9
    are dead from their first rows while lanes 10 to 15 have not started: they
    vote alive until they have."""
    msc = efm.scalar_scoring(*scheme)
    s = rand_seq(random.Random(0x5EED), 60, b"ACGT")
    q, d = b"N" * 100 + s, s
    X = -(scheme[2] + 100 * scheme[3])
    res, cig = check(saln, [q], [d], [(0, 0)], X, str(scheme), scheme, msc)
    assert cig[0] == [(100, "I"), (60, "=")] and int(res["score"][0]) == 300 - X
    res, cig = check(saln, [q], [d], [(0, 0)], X - 1, str(scheme), scheme, msc)
    assert int(res["score"][0]) < 300 - X and cig[0][:1] != [(100, "I")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("default", "open0"))
def test_column_0(saln, name):
    """Leading deletions of 63, 64, 65 rows (around the lanes of a group): (i, 0)
    is unpruned iff X >= -(o + i e)."""
    sc, msc, letters = scoring(saln, name)
    s = rand_seq(random.Random(0x5EED), 200, b"ACGT")
    for g in (63, 64, 65):
        d = b"N" * g + s + rand_seq(random.Random(g), 20, b"ACGT")
        X = -(sc[2] + g * sc[3])
        res, cig = check(saln, [s], [d], [(0, 0)], X, name, sc, msc)
        assert cig[0] == [(g, "D"), (200, "=")] and int(res["score"][0]) == 1000 - X
        res, cig = check(saln, [s], [d], [(0, 0)], X - 1, name, sc, msc)
        assert int(res["score"][0]) < 1000 - X and cig[0][:1] != [(g, "D")]


# ------------------------------------------------------------------ 6. direction, the scalar engine, large X, no X
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_direction_left(saln, name):
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0x1EF8)
    for n, m, X in ((40, 60, 15), (300, 90, 40), (11, 11, 0), (5, 0, 9), (150, 700, 25)):
        q = rand_seq(rng, n, letters)
        d = anchored(rng, q[::-1], m, letters)[::-1]       # related at the right ends
        want = efm.left_coords(expect(q[::-1], d[::-1], X, name, msc)[0], n, m)
        rec, cigar = saln.extend_align(q, d, scoring=sc, direction="left", xdrop=X)
        assert tuple(int(v) for v in rec)[:7] == want.record()[:7] and cigar == want.cigar
        assert saln.alignment_score(q, d, (rec, cigar), sc) == want.score
        rrec, rcigar = saln.extend_align(q[::-1], d[::-1], scoring=sc, xdrop=X)
        assert int(rrec["score"]) == want.score and rcigar == cigar[::-1]
        assert int(rrec["reserved"]) == int(rec["reserved"]) > 0


def mixed_batch(seed):
    rng = random.Random(seed)
    qs = [rand_seq(rng, rng.randint(0, 60), b"ACGT") for _ in range(150)]
    ds = [anchored(rng, q, rng.randint(0, 60), b"ACGT") for q in qs]
    pairs = [(k, k) for k in range(150)]
    for n in (150, 161, 300, 512, 700, 1024):
        pairs.append((len(qs), len(ds)))
        qs.append(rand_seq(rng, n, b"ACGT"))
        ds.append(anchored(rng, qs[-1], 150, b"ACGT") + rand_seq(rng, 150, b"ACGT"))
    return qs, ds, pairs


@pytest.mark.gpu
def test_match_mismatch_matrix_equals_the_scalar_engine(saln):
    table = [[5 if a == b else -4 for b in range(4)] for a in range(4)]
    sm = saln.SubstitutionMatrix(b"ACGT", table, -8, -6)
    qs, ds, pairs = mixed_batch(0xEF09)
    for X in (0, 12, 45):
        for cigar in (True, False):
            want, wcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=DEFAULT, cigar=cigar, xdrop=X)
            got, gcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sm, cigar=cigar, xdrop=X)
            assert (got == want).all()                    # `reserved` too: the same steps
            assert [gcig.words(k).tolist() for k in range(len(pairs))] == \
                [wcig.words(k).tolist() for k in range(len(pairs))]
    assert int((want["score"] != 0).sum()) > 60


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_large_x_is_plain_extension(saln, name):
    """Nothing real is pruned: records (but the steps) and words are those of
    ends_free_align_batch(mode=EXTEND), and every pair runs all its rows."""
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0x1A26F)
    qs = [rand_seq(rng, n, letters) for n in (7, 33, 160, 161, 400, 513, 1024, 90)]
    ds = [anchored(rng, q, m, letters) for q, m in zip(qs, (40, 33, 120, 5, 200, 64, 150, 700))]
    pairs = [(k, k) for k in range(len(qs))] + [(0, 7), (7, 0)]
    for cigar in (True, False):
        want, wcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, cigar=cigar)
        X = max(model.no_drop(len(qs[a]), len(ds[b]), msc) for a, b in pairs)
        got, gcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, cigar=cigar, xdrop=X)
        for f in want.dtype.names[:7]:
            assert (got[f] == want[f]).all(), f
        assert [gcig.words(k).tolist() for k in range(len(pairs))] == \
            [wcig.words(k).tolist() for k in range(len(pairs))]
        assert (want["reserved"] == 0).all()
        for k, (a, b) in enumerate(pairs):
            # the last lane with a real column runs row m at step m + (its index); the vote after
            # the next step ends the loop, unless the loop's own m + lanes - 1 steps end first
            lanes, cols = saln.ends_free.pair_geometry(len(qs[a]))
            used = -(-len(qs[a]) // cols)
            assert int(got["reserved"][k]) == min(len(ds[b]) + used, len(ds[b]) + lanes - 1)
    assert int((want["score"] > 0).sum()) >= 6


@pytest.mark.gpu
def test_without_xdrop_reserved_stays_0(saln):
    qs, ds, pairs = mixed_batch(0x0E20)
    for kw in ({}, {"xdrop": None}):
        res, _ = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=OPEN0, **kw)
        assert (res["reserved"] == 0).all() and (saln.xdrop_steps(res) == 0).all()
    rec, _ = saln.extend_align(qs[150], ds[150], xdrop=None)
    assert int(rec["reserved"]) == 0
    rec, _ = saln.extend_align(qs[150], ds[150], xdrop=50)
    assert int(rec["reserved"]) > 0
