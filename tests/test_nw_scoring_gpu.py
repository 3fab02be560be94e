"""GPU parity under custom scoring schemes: every NW entry point against the
CPU oracle run with the same scheme (oracle/refcpu.c ref_nw_fill_s), bit for
bit - score, end states, panic status, printed flag, the first printed
alignment op for op and, where the shape allows, every parent code.

The schemes (nw_check.SCHEMES) sit on the edges of the engine's int16 / int32
range guards; the guard-edge tests find each edge by asking created plans what
their execute will launch (NwPlan.pair_path), never by restating a guard."""
import numpy as np
import pytest

from nw_check import (DECISIONS, KINDS, PANIC, POSITIVE_EXTEND, SCHEMES, SENTINEL_SCHEME, PlanRun, assert_batch, csr, expand,
                      make_pair, rand_seq)
from nw_check import scheme_seed as _seed

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------- (a) variant sweep
SWEEP_SHAPES = [(1, 1), (19, 19), (150, 150), (152, 300), (153, 160), (160, 400), (200, 180),
                (257, 64), (513, 70), (1025, 40), (40, 2000)]


@pytest.mark.parametrize("scheme", list(SCHEMES), ids=lambda s: "_".join(map(str, s)))
def test_variant_sweep(saln, oracle, scheme):
    """Every scheme over shapes of every fill variant and three pair kinds,
    through n_w_align and dense_mask one pair at a time, then all of them as
    one nw_align_batch."""
    rng = np.random.default_rng(_seed(scheme))
    pairs = [make_pair(rng, kind, lq, ld) for lq, ld in SWEEP_SHAPES for kind in KINDS[:3]]
    for q, d in pairs:
        o = oracle.nw(q, d, literal_dfs=False, scoring=scheme)
        r = saln.n_w_align(q, d, scoring=scheme)
        tag = (scheme, len(q), len(d))
        assert (r.score, r.end_states, r.panics, r.printed) == \
            (o.score, o.end_states, o.panics, o.first_ops is not None), tag
        if o.first_ops is not None:
            assert expand(r.cigar) == o.first_ops, tag
        dm = saln.dense_mask(q, d, scheme)
        if not np.array_equal(dm, o.dense_mask):
            bad = np.argwhere(dm != o.dense_mask)
            raise AssertionError(f"{tag}: {len(bad)} mask bytes differ, first at {bad[:4].tolist()}")
    queries, dbs = [q for q, _ in pairs], [d for _, d in pairs]
    res, cig = saln.nw_align_batch(queries, dbs, pairs=[(k, k) for k in range(len(pairs))],
                                   scoring=scheme)
    want = oracle.check_pairs(*csr(queries), *csr(dbs), scoring=scheme)
    assert_batch(res, cig.words, want, scheme)


# ------------------------------------------------------------------ regressions
def _assert_pairs(saln, oracle, scheme, pairs):
    """Each pair alone (n_w_align) and all of them as one batch."""
    for q, d in pairs:
        o = oracle.nw(q, d, literal_dfs=False, scoring=scheme)
        r = saln.n_w_align(q, d, scoring=scheme)
        assert (r.score, r.end_states, r.panics, r.printed) == \
            (o.score, o.end_states, o.panics, o.first_ops is not None), (scheme, len(q), len(d))
        if o.first_ops is not None:
            assert expand(r.cigar) == o.first_ops, (scheme, len(q), len(d))
    queries, dbs = [q for q, _ in pairs], [d for _, d in pairs]
    res, cig = saln.nw_align_batch(queries, dbs, pairs=[(k, k) for k in range(len(pairs))],
                                   scoring=scheme)
    assert_batch(res, cig.words, oracle.check_pairs(*csr(queries), *csr(dbs), scoring=scheme),
                 scheme)


@pytest.mark.parametrize("scheme,shapes", [
    (SENTINEL_SCHEME, [(1, 1), (2, 3), (5, 1), (8, 8), (1, 12)]),
    ((8, -8, -16, -12), [(10, 190), (3, 250), (170, 200), (20, 300)]),
    ((5, -4, -8, -20), [(10, 150), (4, 300), (200, 120)]),
])
def test_regression_narrow_query_rebasing_frame(saln, oracle, scheme, shapes):
    """A query much narrower than its lane group once passed the single-frame
    guard on its own width; the launch, which judges the group's whole width,
    then took the rebasing frame although packed_ok_rebase refuses these
    schemes: 1 x 1 under (5,-4,-8,-600) scored 98,300 instead of -4."""
    rng = np.random.default_rng(_seed(scheme) + 1)
    _assert_pairs(saln, oracle, scheme,
                  [make_pair(rng, kind, lq, ld) for lq, ld in shapes for kind in KINDS[:3]])


@pytest.mark.parametrize("scheme,shapes", [
    ((1, 0, 0, 0), [(40, 2000), (150, 700), (160, 1300), (250, 1300)]),
    ((1, 0, -1, 0), [(40, 2000), (152, 625)]),
    ((2, -3, -5, -2), [(152, 1227), (150, 630)]),
])
def test_regression_small_penalties_long_db(saln, oracle, scheme, shapes):
    """Under small penalties the int16 range admits more db rows than a
    single-frame launch can stage in LDS at 4 B a row: these pairs failed with
    E_HIP (launch_fill: invalid argument) before the single-frame guard took
    the staged rows into account."""
    rng = np.random.default_rng(_seed(scheme) + 2)
    _assert_pairs(saln, oracle, scheme,
                  [make_pair(rng, kind, lq, ld) for lq, ld in shapes for kind in KINDS[:3]])


# --------------------------------------------------------------- (b) guard edges
EDGE_SCHEMES = [(5, -4, -8, -6), (2, -3, -5, -2), (8, -8, -16, -12), (12, -4, -20, -16),
                (5, -4, -8, -20), (16, 0, -30, -40), (5, -4, -6800, -1), (8, -8, -8, -7)]
EDGE_WIDTHS = [150, 152, 160, 256, 512, 1024]
LD_CAP = 4096  # an edge at or beyond it is the staged-row bound, not a range guard
def _path_at(saln, scheme, lq, ld, cache):
    if ld not in cache:
        n = 64
        qo = np.arange(n + 1, dtype=np.uint64) * np.uint64(lq)
        do = np.arange(n + 1, dtype=np.uint64) * np.uint64(ld)
        plan = saln.NwPlan(qo, do, pairs=np.stack([np.arange(n)] * 2, 1), scoring=scheme)
        cache[ld] = plan.pair_path(0)
        plan.close()
    return cache[ld]


def _find_edge(saln, scheme, lq, decision, cache):
    """(edge, pred): the largest ld in [1, LD_CAP] at which the decision holds
    on the fill variant that takes it first (past the edge the pairs move to
    another variant, frame or body), or None if it never holds on the scan
    grid or still does at LD_CAP."""
    grid = sorted({1, 2, 3, 5, 8, 12, 18, 24, 36, 48, 64, 90, 100, 128, 150, 180, 256, 360, 450,
                   512, 600, 720, 1024, 1200, 1448, 2048, 2500, 2896, 3500, LD_CAP})
    first = [ld for ld in grid if decision(_path_at(saln, scheme, lq, ld, cache))]
    if not first:
        return None
    variant = cache[first[0]].variant
    pred = lambda p: decision(p) and p.variant == variant  # noqa: E731
    holds = [ld for ld in grid if pred(cache[ld])]
    if holds[-1] == LD_CAP:
        return None
    lo, hi = holds[-1], grid[grid.index(holds[-1]) + 1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(_path_at(saln, scheme, lq, mid, cache)):
            lo = mid
        else:
            hi = mid
    return lo, pred


def _scheme_edges(saln, saln_opt, scheme):
    """[(decision, width, edge, path at the edge, path past it)] of one scheme,
    from created plans alone (nothing executes)."""
    saln_opt("nw.wide_min_pairs", 0)  # 513..1,024-column queries stay on the 64-lane packed fill
    out = []
    for tab in (3, 1, 2):
        saln_opt("nw.pk_tab", tab)
        for lq in EDGE_WIDTHS:
            cache = {}
            for name, (need_tab, decision) in DECISIONS.items():
                if need_tab != tab:
                    continue
                hit = _find_edge(saln, scheme, lq, decision, cache)
                if hit is None:
                    continue
                edge, pred = hit
                inside, outside = cache[edge], cache[edge + 1]
                assert pred(inside) and not pred(outside) and inside != outside, \
                    (scheme, lq, name, edge, inside, outside)
                out.append((name, tab, lq, edge, inside, outside))
    return out


@pytest.mark.parametrize("scheme", EDGE_SCHEMES, ids=lambda s: "_".join(map(str, s)))
def test_guard_edges(saln, oracle, saln_opt, scheme):
    """For each query width and each launch decision the scheme reaches, the
    last db length on which the engine takes it (bisected over created plans)
    and the first one past it: both sides execute five pair kinds that push
    the frame's extremes, and equal the oracle."""
    rng = np.random.default_rng(_seed(scheme))
    edges = _scheme_edges(saln, saln_opt, scheme)
    for name, tab, lq, edge, inside, outside in edges:
        saln_opt("nw.pk_tab", tab)
        for ld, path in ((edge, inside), (edge + 1, outside)):
            pairs = [make_pair(rng, kind, lq, ld) for kind in KINDS]
            with PlanRun(saln, [q for q, _ in pairs], [d for _, d in pairs], scheme) as run:
                got = run.plan.pair_path(0)
                # (five pairs instead of 64: the same launch decisions)
                assert (got.variant, got.packed, got.rebase, got.table) == \
                    (path.variant, path.packed, path.rebase, path.table), (scheme, lq, ld)
                run.run()
                want = oracle.check_pairs(run.qs, run.qo, run.ds, run.do, scoring=scheme)
                assert_batch(run.res, run.words, want, (scheme, name, lq, ld, path))
    print(f"guard edges {scheme}: {[(n, w, e) for n, _, w, e, _, _ in edges]}")


def test_guard_edges_cover_every_decision(saln, saln_opt):
    """Each launch decision has an edge below LD_CAP, at some width, under at
    least two of the schemes: test_guard_edges executes both sides of every
    edge that this same search finds, so each decision is tested on both
    sides under at least two schemes.  Stands alone (creation only)."""
    seen = {}
    for scheme in EDGE_SCHEMES:
        for name, _, lq, edge, _, _ in _scheme_edges(saln, saln_opt, scheme):
            seen.setdefault(name, {}).setdefault(scheme, []).append((lq, edge))
    for name, by_scheme in seen.items():
        for scheme, edges in by_scheme.items():
            print(f"edge table: {name:15s} {scheme}: " +
                  ", ".join(f"W={w}: {e}" for w, e in edges))
    for name in DECISIONS:
        assert len(seen.get(name, {})) >= 2, (name, seen.get(name))


# -------------------------------------------------------------------- (c) plans
PLAN_SCHEMES = [(5, -4, -8, -6), (2, -3, -5, -2), (1, 0, 0, 0), (8, -8, -16, -12),
                SENTINEL_SCHEME, (6, 2, -8, -6)] + POSITIVE_EXTEND
_ragged_cache: dict = {}


def _ragged(oracle, scheme):
    """2,000 pairs, sides 0..400, an N in 1 % of the sequences; the oracle's
    results once per scheme."""
    if scheme not in _ragged_cache:
        rng = np.random.default_rng(2000 + PLAN_SCHEMES.index(scheme))
        n = 2000
        seqs = []
        for side in range(2):
            out = []
            for k in range(n):
                s = bytearray(rand_seq(rng, int(rng.integers(0, 401))))
                if s and rng.random() < 0.01:
                    s[int(rng.integers(len(s)))] = ord("N")
                out.append(bytes(s))
            seqs.append(out)
        want = oracle.check_pairs(*csr(seqs[0]), *csr(seqs[1]), scoring=scheme)
        _ragged_cache[scheme] = (seqs[0], seqs[1], want)
    return _ragged_cache[scheme]


@pytest.mark.parametrize("scheme", PLAN_SCHEMES, ids=lambda s: "_".join(map(str, s)))
def test_ragged_plan_sync_full_and_score_only(saln, oracle, scheme):
    queries, dbs, want = _ragged(oracle, scheme)
    with PlanRun(saln, queries, dbs, scheme) as run:
        run.run()
        assert_batch(run.res, run.words, want, (scheme, "sync"))
    with PlanRun(saln, queries, dbs, scheme, score_only=True) as run:
        run.run()
        assert_batch(run.res, None, want, (scheme, "score only"), score_only=True)
    with PlanRun(saln, queries, dbs, scheme, full=True) as run:
        run.run()
        assert_batch(run.res, run.words, want, (scheme, "full codes"))
        rng = np.random.default_rng(7)
        filled = [k for k in range(len(queries)) if queries[k] and dbs[k]]
        for k in rng.choice(filled, 50, replace=False):
            o = oracle.nw(queries[int(k)], dbs[int(k)], literal_dfs=False, scoring=scheme)
            assert np.array_equal(run.plan.dense_mask(int(k)), o.dense_mask), (scheme, int(k))


@pytest.mark.parametrize("tab", [0, 1, 2, 3])
@pytest.mark.parametrize("scheme", PLAN_SCHEMES, ids=lambda s: "_".join(map(str, s)))
def test_ragged_plan_pipelined(saln, oracle, saln_opt, scheme, tab):
    """The pipelined plan under each packed body (nw.pk_tab), two executes in
    flight: the table bodies' end values and CIGARs, and the deferred
    fallback launches of the waves that hold an N."""
    saln_opt("nw.pk_tab", tab)
    queries, dbs, want = _ragged(oracle, scheme)
    with PlanRun(saln, queries, dbs, scheme, pipelined=True) as run:
        for step in range(2):
            run.run()
            assert_batch(run.res, run.words, want, (scheme, "pipelined", tab, step))


# --------------------------------------------------------------- (d) all-vs-all
@pytest.mark.parametrize("profile", [1, 0])
@pytest.mark.parametrize("ld_max", [700, 500, 170])
@pytest.mark.parametrize("scheme", [(2, -3, -5, -2), (8, -8, -16, -12), SENTINEL_SCHEME,
                                    (8, -8, -8, -7)] + POSITIVE_EXTEND,
                         ids=lambda s: "_".join(map(str, s)))
def test_all_vs_all(saln, oracle, saln_opt, scheme, ld_max, profile):
    """64 queries x 48 dbs.  The longest db decides the classes' launches:
    700 rows keep the 16 x 10 class, 500 form the 8 x 19 class with query
    profiles, in one int16 frame under (2,-3,-5,-2) and in the rebasing one
    under (8,-8,-8,-7); 170 rows fit one frame under (8,-8,-16,-12) too."""
    saln_opt("nw.avsa_profile", profile)
    rng = np.random.default_rng(64 + ld_max)
    ql = [152, 153, 160, 161, 1, 300] + [int(x) for x in rng.integers(1, 301, 58)]
    dl = [1, ld_max] + [int(x) for x in rng.integers(1, ld_max + 1, 46)]
    queries = [rand_seq(rng, n) for n in ql]
    dbs = [rand_seq(rng, n) for n in dl]
    queries[7] = queries[7][:-1] + b"N"
    dbs[5] = b"N" + dbs[5][1:]
    scores, status = saln.nw_score_all_vs_all(queries, dbs, scoring=scheme)
    pq = [q for _ in dbs for q in queries]  # db outer, query inner
    pd = [d for d in dbs for _ in queries]
    want = oracle.check_pairs(*csr(pq), *csr(pd), scoring=scheme)
    assert len(want.score) == 3072
    got = scores.reshape(-1)
    bad = np.flatnonzero(got != want.score)
    assert bad.size == 0, (scheme, [(int(k) % 64, int(k) // 64, ql[int(k) % 64], dl[int(k) // 64],
                                     int(got[k]), int(want.score[k])) for k in bad[:8]])
    assert np.array_equal(status.reshape(-1) == PANIC, want.panics)


# --------------------------------------------------------------- (e) long pairs
_long_cache: dict = {}


def _long_pair(oracle, name, scheme):
    from sequencealigning_amd import synth
    key = (name, scheme)
    if key not in _long_cache:
        rng = np.random.default_rng(len(name))
        if name == "mut_5000":
            q, d = synth.mut_pair(5000, 0.05, 0x5C0)
        else:
            lq, ld = {"iid_3000x6000": (3000, 6000), "iid_700x650": (700, 650),
                      "iid_2000x300": (2000, 300)}[name]
            q, d = rand_seq(rng, lq), rand_seq(rng, ld)
        _long_cache[key] = (q, d, oracle.nw_first_linear(q, d, scoring=scheme)[:4])
    return _long_cache[key]


def _assert_long(r, want, tag):
    sc, es, pan, first = want
    assert (r.score, r.end_states, r.status == PANIC, r.printed) == \
        (sc, es, pan, first is not None), tag
    if first is not None:
        assert expand(r.cigar) == first, tag


LONG_CASES = [("mut_5000", (2, -3, -5, -2)), ("mut_5000", (1, 0, -1, 0)),
              ("iid_3000x6000", (2, -3, -5, -2)), ("iid_3000x6000", (1, 0, -1, 0)),
              ("iid_700x650", SENTINEL_SCHEME), ("iid_2000x300", SENTINEL_SCHEME)] + \
    [(name, s) for s in POSITIVE_EXTEND for name in ("mut_5000", "iid_2000x300")]


@pytest.mark.parametrize("stripes", [(1, 0), (0, 1), (0, 2)], ids=["packed", "rows_k1", "rows_k2"])
@pytest.mark.parametrize("name,scheme", LONG_CASES)
def test_long_pair_stripes(saln, oracle, saln_opt, name, scheme, stripes):
    """Column stripes: packed where the scheme allows it (nw.stripe_pk = 1),
    the row fill at one and two columns per lane, each with the speculative
    walks on and off.  A positive extend has no packed stripes: forced, the
    plan still reports the row fill, and the pair runs on it."""
    q, d, want = _long_pair(oracle, name, scheme)
    saln_opt("nw.stripe_pk", stripes[0])
    saln_opt("nw.rows_k", stripes[1])
    if stripes[0] and scheme[3] > 0:
        plan = saln.NwPlan(*(np.array([0, len(s)], np.uint64) for s in (q, d)), pairs=[(0, 0)],
                           scoring=scheme)
        path = plan.pair_path(0)
        plan.close()
        assert not path.packed and not path.stripe_pk, (name, scheme, path)
    for spec in (1, 0):
        saln_opt("nw.spec", spec)
        _assert_long(saln.n_w_align(q, d, scoring=scheme), want, (name, scheme, stripes, spec))


@pytest.mark.parametrize("name,scheme", LONG_CASES)
def test_long_pair_spans(saln, oracle, name, scheme):
    from sequencealigning_amd.span import nw_align_long_spans
    q, d, want = _long_pair(oracle, name, scheme)
    _assert_long(nw_align_long_spans(q, d, 3, scoring=scheme, band_rows=512), want, (name, scheme))
