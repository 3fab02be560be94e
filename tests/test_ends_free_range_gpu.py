"""GPU: the ends-free engine at the accepted edge of its range guard,
(len_q + len_db + 2) * max|parameter| (+ X) < 2^30: the four modes and X-drop
through the class fills, the chunked fill, the tiled replay and the chunked
X-drop fill, under schemes whose largest magnitude is the largest the guard
accepts for the pair (test_ends_free_range.py has the cases and the conditions
that keep them honest).  Every comparison is exact against the plain models
(ends_free_model.py, xdrop_model.py), which compute in int64 with -2^60 as
-infinity: the whole record, the CIGAR word for word, alignment_score, and the
X-drop fills' `reserved` within steps_bound.

The scheme depends on the pair's lengths, so every shape is a call of its own,
of three pairs (the three relations of d to q)."""
import numpy as np
import pytest

import ends_free_model as model
import test_ends_free_range as R
import xdrop_long_model as lm
import xdrop_model

EXTEND = model.EXTEND


def plan_results(saln, qs, ds, pairs, sc, X, mode=EXTEND):
    """The records of EndsFreePlan.execute (score only; X: None or the X-drop)."""
    import torch
    from sequencealigning_amd import _lib
    qb, qo = saln.pack_csr(qs)
    db, do = saln.pack_csr(ds)
    plan = saln.EndsFreePlan(qo, do, pairs, mode=mode, scoring=sc, xdrop=X)
    dq = torch.from_numpy(np.concatenate([qb, np.zeros(16, np.uint8)])).cuda()
    dd = torch.from_numpy(np.concatenate([db, np.zeros(16, np.uint8)])).cuda()
    out = torch.full((plan.n_pairs * 8,), 77, dtype=torch.int32, device="cuda")
    plan.execute(dq, dd, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE)
    plan.close()
    return got


def batch_of(n, m, name):
    three = R.relations(n, m, R.is_matrix(name))
    return [q for q, _ in three], [d for _, d in three], [(k, k) for k in range(len(three))]


def ends_of(a):
    """The score-only record of the model's alignment."""
    return (a.score, 0, -1, a.q_end, -1, a.db_end, 0, 0)


def same_alignments(saln, res, cig, qs, ds, want, sc, tag):
    assert len(res) == len(cig) == len(want)
    for k, a in enumerate(want):
        assert tuple(int(v) for v in res[k])[:7] == a.record()[:7], (tag, k, res[k], a.record())
        assert cig.words(k).tolist() == model.cigar_words(a.cigar), (tag, k)
        assert saln.alignment_score(qs[k], ds[k], (res[k], cig[k]), sc) == a.score, (tag, k)


def same_ends(res, cig, want, tag):
    for k, a in enumerate(want):
        assert tuple(int(v) for v in res[k])[:7] == ends_of(a)[:7] and cig[k] == [], (tag, k, res[k], ends_of(a))


# ------------------------------------------------------------------ 1. the four modes
@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCHEMES)
@pytest.mark.parametrize("mode", R.MODES)
def test_class_fills_at_the_edge(saln, mode, name):
    """Tiny pairs (P near 2^28: lane 0's border product of the steps past the
    last row leaves int32) and every class with and without pad columns, with
    CIGAR, score only, through EndsFreePlan and through the long entry point."""
    for n, m in R.TINY + R.CLASS:
        P = R.edge_p(n, m)
        sc = R.engine_scoring(saln, name, P)
        qs, ds, pairs = batch_of(n, m, name)
        want = [R.expect(q, d, mode, name, P) for q, d in zip(qs, ds)]
        tag = (n, m, mode, name)
        res, cig = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=sc)
        same_alignments(saln, res, cig, qs, ds, want, sc, tag)
        assert (res["reserved"] == 0).all()
        sres, scig = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=sc, cigar=False)
        same_ends(sres, scig, want, tag)
        assert (plan_results(saln, qs, ds, pairs, sc, None, mode=mode) == sres).all(), tag
        lres, lcig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sc)
        same_alignments(saln, lres, lcig, qs, ds, want, sc, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCHEMES)
@pytest.mark.parametrize("mode", R.MODES)
def test_chunked_fill_and_replay_at_the_edge(saln, mode, name):
    """Two and three chunks (the third with pad columns): the chunked fill with
    codes and score only, and the tiled replay with tiles of 64 rows, so that
    several tiles, boundary columns and checkpoint rows hold edge values."""
    from sequencealigning_amd import _lib
    for n, m in R.CHUNKED:
        assert saln.ends_free.pair_path_long(n, m) == (1, -(-n // 1024))
        P = R.edge_p(n, m)
        sc = R.engine_scoring(saln, name, P)
        qs, ds, pairs = batch_of(n, m, name)
        want = [R.expect(q, d, mode, name, P) for q, d in zip(qs, ds)]
        tag = (n, m, mode, name)
        res, cig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sc)
        same_alignments(saln, res, cig, qs, ds, want, sc, tag)
        sres, scig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sc, cigar=False)
        same_ends(sres, scig, want, tag)
        with _lib.options(**{"ends_free.tile_rows": 64}):
            rres, rcig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sc, replay=True)
        same_alignments(saln, rres, rcig, qs, ds, want, sc, tag + ("replay",))


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCHEMES)
@pytest.mark.parametrize("mode", R.MODES)
def test_tall_db_at_the_edge(saln, mode, name):
    """70 x 65,001, one row above the class limit: the chunked fill over 65,064
    steps, score only against the model's rolling rows."""
    n, m = R.TALL
    assert saln.ends_free.pair_path_long(n, m) == (1, 1)
    P = R.edge_p(n, m)
    sc = R.engine_scoring(saln, name, P)
    qs, ds, pairs = batch_of(n, m, name)
    res, cig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sc, cigar=False)
    for k in range(len(pairs)):
        score, q_end, db_end = R.expect_ends(qs[k], ds[k], mode, name, P)
        assert tuple(int(v) for v in res[k]) == (score, 0, -1, q_end, -1, db_end, 0, 0), (k, mode, name)


# ------------------------------------------------------------------ 2. X-drop
def xdrop_forms(saln, qs, ds, pairs, X, name, P, sc, batch, bound, tag, chunked=False):
    """With words and score only through `batch`: record, words, alignment_score,
    and the steps between max(L, 1) (chunked: 1) and bound(q, d, L)."""
    want = [R.expect_x(q, d, X, name, P) for q, d in zip(qs, ds)]
    res, cig = batch(qs, ds, pairs, scoring=sc, xdrop=X)
    same_alignments(saln, res, cig, qs, ds, [a for a, _ in want], sc, tag)
    sres, scig = batch(qs, ds, pairs, scoring=sc, xdrop=X, cigar=False)
    same_ends(sres, scig, [a for a, _ in want], tag)
    for k, (a, L) in enumerate(want):
        steps, most = int(res["reserved"][k]), bound(qs[k], ds[k], L)
        print(tag, k, "score", a.score, "L", L, "steps", steps, "bound", most)
        assert (1 if chunked else max(L, 1)) <= steps <= most, (tag, k, steps, L, most)
    assert (sres["reserved"] == res["reserved"]).all(), tag     # the same fill, with and without codes
    return sres


@pytest.mark.gpu
@pytest.mark.parametrize("xkind", R.XKINDS)
@pytest.mark.parametrize("name", R.SCHEMES)
def test_xdrop_at_the_edge(saln, name, xkind):
    """Extension under X = 0, X = P and X the guard's remainder above a halved P
    (about 2^29); what each prunes is the model's to say.  The class fills in
    their three forms (the tiny pairs too: their border product leaves int32
    here as well), and 1,030 x 70 through the chunked X-drop fill."""
    for n, m in R.XDROP_SHAPES:
        P, X = R.x_case(n, m, xkind)
        sc = R.engine_scoring(saln, name, P)
        qs, ds, pairs = batch_of(n, m, name)
        lanes = saln.ends_free.pair_geometry(n)[0]

        def batch(qs, ds, pairs, **kw):
            return saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, **kw)

        sres = xdrop_forms(saln, qs, ds, pairs, X, name, P, sc, batch,
                           lambda q, d, L: xdrop_model.steps_bound(len(d), L, lanes), (n, m, name, xkind))
        assert (plan_results(saln, qs, ds, pairs, sc, X) == sres).all(), (n, m, name, xkind)
    n, m = R.XDROP_LONG
    P, X = R.x_case(n, m, xkind)
    sc = R.engine_scoring(saln, name, P)
    msc = R.model_scoring(name, P)
    qs, ds, pairs = batch_of(n, m, name)
    assert saln.ends_free.pair_path_long(n, m) == (1, 2)
    xdrop_forms(saln, qs, ds, pairs, X, name, P, sc, saln.xdrop_extend_long_batch,
                lambda q, d, L: lm.steps_bound(lm.schedule(q, d, X, msc)[2]), (n, m, name, xkind), chunked=True)


@pytest.mark.gpu
def test_the_models_agree_where_nothing_is_pruned(saln):
    """The guard's remainder as X prunes nothing real of an identical prefix:
    the X-drop record is plain extension's, on the engine as in the models."""
    for n, m in ((10, 10), (300, 300)):
        P, X = R.x_case(n, m, "rest")
        q, d = R.relations(n, m, False)[0]
        a, L = R.expect_x(q, d, X, "all", P)
        assert a == R.expect(q, d, EXTEND, "all", P) and L == m and a.score == m * P
        res, cig = saln.ends_free_align_batch([q], [d], mode=EXTEND, scoring=R.SCALAR["all"](P), xdrop=X)
        pres, pcig = saln.ends_free_align_batch([q], [d], mode=EXTEND, scoring=R.SCALAR["all"](P))
        assert tuple(int(v) for v in res[0])[:7] == tuple(int(v) for v in pres[0])[:7] == a.record()[:7]
        assert cig.words(0).tolist() == pcig.words(0).tolist()
        assert np.asarray(res["reserved"])[0] > 0
