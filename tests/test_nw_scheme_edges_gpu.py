"""Guard edges along the scoring-scheme axis.  test_guard_edges
(test_nw_scoring_gpu.py) fixes a scheme and walks the db length, so the guard
terms that bind only under large scores are never stood on: the rebasing
frame's range and sentinel-floor terms, the packed stripes' range term and the
byte edges of the table bodies' bonuses.  Here the shape is fixed and one
scheme parameter t is walked along a family t -> scheme; the edge is the last
t at which a launch decision holds, asked of created plans
(NwPlan.pair_path), never by restating a guard.  Both sides of every edge
execute six pair kinds against the CPU oracle under the same scheme, bit for
bit: score, end states, panic status, printed flag, every CIGAR word."""
import numpy as np
import pytest

from nw_check import (DECISIONS, KINDS, PANIC, PlanRun, assert_batch, expand, make_pair,
                      scheme_seed)

pytestmark = pytest.mark.gpu

EDGE_KINDS = KINDS + ("suffix",)
T_CAP = 256  # a decision that still holds here has no edge on the family
T_GRID = [1, 2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 90, 128, 181, T_CAP]

FAMILIES = {
    "5,-4,-8,-t": lambda t: (5, -4, -8, -t),        # the extend alone
    "t,t-9,-8,-6": lambda t: (t, t - 9, -8, -6),     # the default's penalty, larger bonuses
    "t,t-5,-5,-2": lambda t: (t, t - 5, -5, -2),
    "t,t-16,-8,-7": lambda t: (t, t - 16, -8, -7),   # pen = 32, the packed fills' largest
    "t,t-16,0,-40": lambda t: (t, t - 16, 0, -40),   # the bonus byte 2 m + 160
    "t,t-16,0,-45": lambda t: (t, t - 16, 0, -45),
}
# decision -> (nw.pk_tab, nw.stripe_pk, predicate on a PairPath)
SETTINGS = {name: (tab, -1, pred) for name, (tab, pred) in DECISIONS.items()}
SETTINGS["packed stripes"] = (3, 1, lambda p: p.stripe_pk)
WIDE = [(150, 700), (256, 700), (512, 700), (1024, 700)]
# (decision, family, shapes lq x ld): shapes at which the family is expected
# to leave the decision below T_CAP; the edges themselves come from pair_path
CASES = [
    ("single frame", "5,-4,-8,-t", [(150, 12), (160, 100)]),
    ("single frame", "t,t-9,-8,-6", [(150, 8)]),
    ("rebasing frame", "t,t-9,-8,-6", WIDE),
    ("rebasing frame", "t,t-5,-5,-2", WIDE),
    ("rebasing frame", "t,t-16,-8,-7", WIDE),
    ("rebasing frame", "5,-4,-8,-t", [(150, 700)]),  # the sentinel-floor term
    ("table scale 2", "t,t-16,0,-40", [(150, 8)]),
    ("table scale 2", "t,t-16,0,-45", [(150, 8)]),
    ("row profiles", "t,t-16,0,-40", [(150, 8)]),
    ("row profiles", "t,t-16,0,-45", [(150, 8)]),
    ("table scale 4", "5,-4,-8,-t", [(150, 12)]),
    ("table scale 4", "t,t-9,-8,-6", [(150, 12)]),
    # (1,300 columns leave the packed stripes where row 0 reaches the sentinel, 1,100 earlier)
    ("packed stripes", "5,-4,-8,-t", [(1300, 600), (1100, 600)]),
    ("packed stripes", "t,t-9,-8,-6", [(1300, 600)]),
]


def _set_options(saln_opt, name):
    tab, stripe_pk, _ = SETTINGS[name]
    saln_opt("nw.wide_min_pairs", 0)  # 513..1,024-column queries stay on the 64-lane packed fill
    saln_opt("nw.pk_tab", tab)
    saln_opt("nw.stripe_pk", stripe_pk)


def _path_at(saln, family, lq, ld, t, cache):
    if t not in cache:
        n = 64
        qo = np.arange(n + 1, dtype=np.uint64) * np.uint64(lq)
        do = np.arange(n + 1, dtype=np.uint64) * np.uint64(ld)
        plan = saln.NwPlan(qo, do, pairs=np.stack([np.arange(n)] * 2, 1),
                           scoring=FAMILIES[family](t))
        cache[t] = plan.pair_path(0)
        plan.close()
    return cache[t]


def _find_edge(saln, family, lq, ld, decision, cache):
    """(edge, pred): the largest t in [1, T_CAP] at which the decision holds
    on the fill variant that takes it first, or None if it never holds on the
    scan grid or still does at T_CAP.  Nothing executes."""
    first = [t for t in T_GRID if decision(_path_at(saln, family, lq, ld, t, cache))]
    if not first:
        return None
    variant = cache[first[0]].variant
    pred = lambda p: decision(p) and p.variant == variant  # noqa: E731
    holds = [t for t in T_GRID if pred(cache[t])]
    if holds[-1] == T_CAP:
        return None
    lo, hi = holds[-1], T_GRID[T_GRID.index(holds[-1]) + 1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(_path_at(saln, family, lq, ld, mid, cache)):
            lo = mid
        else:
            hi = mid
    return lo, pred


def _case_edges(saln, name, family, shapes):
    """[(lq, ld, t, path at the edge, path past it)] under the options of
    _set_options(name), from created plans alone."""
    out = []
    for lq, ld in shapes:
        cache = {}
        hit = _find_edge(saln, family, lq, ld, SETTINGS[name][2], cache)
        if hit is None:
            continue
        t, pred = hit
        inside, outside = cache[t], _path_at(saln, family, lq, ld, t + 1, cache)
        assert pred(inside) and not pred(outside) and inside != outside, \
            (name, family, lq, ld, t, inside, outside)
        out.append((lq, ld, t, inside, outside))
    return out


def _key(p):
    return p.variant, p.packed, p.rebase, p.table, p.stripe_pk


@pytest.mark.parametrize("name,family,shapes", CASES, ids=[f"{n}-{f}".replace(" ", "_")
                                                           for n, f, _ in CASES])
def test_scheme_axis_edges(saln, oracle, saln_opt, name, family, shapes):
    """Both sides of each edge of one decision along one family: six pair
    kinds through a plan whose pair_path equals the searched one, against
    oracle.check_pairs.  The packed-stripe edges also run each pair through
    n_w_align with the speculative walks on and off, against the linear-memory
    oracle."""
    _set_options(saln_opt, name)
    edges = _case_edges(saln, name, family, shapes)
    assert len(edges) == len(shapes), (name, family, "no edge at",
                                       set(shapes) - {(lq, ld) for lq, ld, *_ in edges})
    for lq, ld, t, inside, outside in edges:
        for tt, path in ((t, inside), (t + 1, outside)):
            scheme = FAMILIES[family](tt)
            rng = np.random.default_rng(scheme_seed(scheme) + lq)
            pairs = [make_pair(rng, kind, lq, ld) for kind in EDGE_KINDS]
            tag = (name, scheme, lq, ld, path)
            with PlanRun(saln, [q for q, _ in pairs], [d for _, d in pairs], scheme) as run:
                # (six pairs instead of 64: the same launch decisions)
                assert _key(run.plan.pair_path(0)) == _key(path), tag
                run.run()
                want = oracle.check_pairs(run.qs, run.qo, run.ds, run.do, scoring=scheme)
                assert_batch(run.res, run.words, want, tag)
            if name != "packed stripes":
                continue
            for q, d in pairs:
                sc, es, pan, first = oracle.nw_first_linear(q, d, scoring=scheme)[:4]
                for spec in (1, 0):
                    saln_opt("nw.spec", spec)
                    r = saln.n_w_align(q, d, scoring=scheme)
                    assert (r.score, r.end_states, r.status == PANIC, r.printed) == \
                        (sc, es, pan, first is not None), (tag, spec)
                    if first is not None:
                        assert expand(r.cigar) == first, (tag, spec)
        print(f"executed edge: {name:15s} {family:13s} {lq} x {ld}: t = {t} "
              f"{FAMILIES[family](t)} | {FAMILIES[family](t + 1)}")


def test_scheme_axis_edges_cover_every_decision(saln, saln_opt):
    """Each of the six launch decisions has a scheme-axis edge under at least
    two families: test_scheme_axis_edges executes both sides of every edge
    that this same search finds.  Stands alone (creation only)."""
    seen = {}
    for name, family, shapes in CASES:
        _set_options(saln_opt, name)
        for lq, ld, t, _, _ in _case_edges(saln, name, family, shapes):
            seen.setdefault(name, {}).setdefault(family, []).append((lq, ld, t))
    for name, by_family in seen.items():
        for family, edges in by_family.items():
            for lq, ld, t in edges:
                print(f"edge table: {name:15s} {family:13s} {lq} x {ld}: t = {t}")
    for name in SETTINGS:
        assert len(seen.get(name, {})) >= 2, (name, seen.get(name))
