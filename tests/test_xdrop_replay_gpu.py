"""GPU: CIGARs of long pairs under X-drop by tiled replay,
saln_ends_free_xdrop_replay_align_batch (ef_xdrop_fill_keep_kernel and
ef_xdrop_tile_fill_kernel in ends_free_xdrop_replay_kernels.hip, the walk of
ends_free_replay_kernels.hip).  Every comparison is
exact: the record's first seven fields and the words against the plain model
(xdrop_model.py) and against xdrop_extend_long_batch without replay on the same
inputs; alignment_score recomputes the score; `reserved` lies within the bound
the schedule model (xdrop_long_model.py) derives from the chunks' windows.  The
inputs' preconditions are asserted from the models, without a device, in
test_the_cases_are_what_they_claim."""
import random

import pytest

import ends_free_model as efm
import test_ends_free_replay as rp
import test_extend_long_gpu as elg
import test_xdrop_long_gpu as xl
import xdrop_long_model as lm
import xdrop_model as model
from test_extend_gpu import DEFAULT, rand_seq
from test_xdrop_long_model import ASYM

EXTEND = efm.EXTEND
CHUNK = 1024
WINDOW_X = {206: [(1, 1027), (961, 1070)], 205: [(1, 1026), (962, 1070)], 230: [(1, 1031), (957, 1070)],
            188: [(1, 1024), (964, 1070)]}


def window_pair():
    """1,100 x 1,070: a 30-column insertion at column 500, so the path stands
    in chunk 1 on rows 1,070 down to 995, and chunk 1's window starts near row
    960 = 15 * 64, on, inside or above a tile edge depending on X."""
    rng = random.Random(0x7113)
    s = rand_seq(rng, 1070, b"ACGT")
    return s[:500] + b"N" * 30 + s[500:], s


def budget_pair():
    rng = random.Random(0xB0D6)
    q = rand_seq(rng, 2100, b"ACGT")
    return q, xl.mutated(rng, q)


def rec7(r):
    return tuple(int(v) for v in r)[:7]


def options(R):
    from sequencealigning_amd import _lib
    return _lib.options(**{"ends_free.tile_rows": R})


def check(saln, qs, ds, pairs, X, name, R, sc=None, msc_key=None):
    """One batch through the replay at tile rows R, against the models and the
    entry point without replay."""
    sc = elg.scoring(saln, name)[0] if sc is None else sc
    with options(R):
        res, cig = saln.xdrop_extend_long_batch(qs, ds, pairs, xdrop=X, scoring=sc, replay=True)
    pres, pcig = saln.xdrop_extend_long_batch(qs, ds, pairs, xdrop=X, scoring=sc)
    assert len(res) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        q, d = qs[a], ds[b]
        want = xl.expect(q, d, X, name)[0]
        tag = (k, len(q), len(d), X, R)
        steps, most = int(res["reserved"][k]), xl.bound(q, d, X, name)
        if len(pairs) < 100:
            print(tag, "steps", steps, "bound", most, "without replay", int(pres["reserved"][k]))
        assert rec7(res[k]) == want.record()[:7], tag
        assert cig.words(k).tolist() == efm.cigar_words(want.cigar), tag
        assert rec7(res[k]) == rec7(pres[k]) and cig.words(k).tolist() == pcig.words(k).tolist(), tag
        assert saln.alignment_score(q, d, (res[k], cig[k]), sc) == want.score, tag
        assert (1 if q and d else 0) <= steps <= most, (tag, steps, most)
        if not xl.is_long(q, d):
            assert steps == int(pres["reserved"][k]), tag     # the class fill, as everywhere
    return res, cig


# ------------------------------------------------------------------ preconditions
def preconditions(key):
    if key == "window":
        q, d = window_pair()
        assert (len(q), len(d)) == (1100, 1070)
        for X, windows in WINDOW_X.items():
            a, alive, L, w = xl.expect(q, d, X, "default")
            assert w == windows, (X, w)
            assert a.cigar == [(500, "="), (30, "I"), (570, "=")] and a.score == 5162
            rows = [i for i, j, _ in rp.path_cells(a) if j > CHUNK]       # the walk in chunk 1
            assert (max(rows), min(rows)) == (1070, 995) and (a.q_end, a.db_end) == (1100, 1070)
        assert WINDOW_X[206][1][0] - 1 == 960 == 15 * 64                 # r0 == lo - 1
        assert all(960 < WINDOW_X[X][1][0] <= 1024 for X in (205, 188))  # the window starts inside the tile
        assert WINDOW_X[230][1][0] <= 960                                 # from a checkpoint row below its top
        assert all(w[0][1] < 1070 for w in WINDOW_X.values())             # rows of chunk 1 past z_0
        a, alive, L, w = xl.expect(q, d, 187, "default")
        assert len(w) == 1 and a.score == 2500 and (a.q_end, a.db_end) == (500, 500) and a.cigar == [(500, "=")]
    elif key == "budget":
        from sequencealigning_amd import ends_free as ef
        assert ef.xdrop_replay_bytes(2100, 2100, 1024) == 689840 and ef.trace_bytes_long(2100, 2100) == 2217600
        assert 600000 < 689840 < 1000000 < 2217600
    else:
        xl.preconditions(key)


@pytest.mark.parametrize("key", ("window", "budget", "diagonal", "dead", "row0", "cheap", "x24", "deletions0",
                                 "deletions1", "deletions2", "mixed"))
def test_the_cases_are_what_they_claim(key):
    preconditions(key)


# ------------------------------------------------------------------ the cases
@pytest.mark.gpu
@pytest.mark.parametrize("R", (64, 1024))
@pytest.mark.parametrize("X", (206, 205, 230, 188, 187))
def test_window_starts_on_in_and_above_a_tile_edge(saln, X, R):
    """Case 1.  At R = 64 the walk visits the tile of rows 961 .. 1,024 of chunk
    1: at X = 206 it starts at the window's top with r0 == lo - 1, at 205 and
    188 the window starts inside it, at 230 it starts from a checkpoint row
    four rows below the window's top.  At 187 the insertion dies: the pair ends
    in chunk 0 of two."""
    preconditions("window")
    q, d = window_pair()
    check(saln, [q], [d], [(0, 0)], X, "default", R)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ("diagonal", "dead", "row0", "cheap", "x24", "deletions0", "deletions1",
                                 "deletions2"))
def test_the_long_x_drop_pairs_through_the_replay(saln, key):
    """Case 2, at R = 64: row 0 live at a later chunk's corner, lo_c = 1 in
    chunk 2, column 0's deletion run across a checkpoint row, a pair that ends
    at a dead chunk."""
    preconditions(key)
    if key == "diagonal":
        runs = [(xl.diagonal_pair(), 60, "default")]
    elif key == "dead":
        runs = [(xl.dead_chunks_pair(), 100, "default")]
    elif key == "row0":
        runs = [(xl.row0_pair(), X, "row0") for X in (xl.ROW0_X, xl.ROW0_X - 1)]
    elif key in ("cheap", "x24"):
        runs = [(xl.crossing_pair(key), X, key) for X in (xl.CROSS_X, xl.CROSS_X - 1)]
    else:
        pair, g = xl.deletion_pairs()[int(key[-1])]
        runs = [(pair, X, "default") for X in (8 + 6 * g, 8 + 6 * g - 1)]
    for (q, d), X, name in runs:
        check(saln, [q], [d], [(0, 0)], X, name, 64)


@pytest.mark.gpu
def test_large_x_is_plain_extensions_replay_word_for_word(saln):
    """Case 3."""
    for name, (q, d) in (("default", xl.diagonal_pair()), ("cheap", xl.crossing_pair("cheap"))):
        sc, msc, _ = elg.scoring(saln, name)
        X = model.no_drop(len(q), len(d), msc)
        with options(64):
            res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=X, scoring=sc, replay=True)
            pres, pcig = saln.ends_free_align_long_batch([q], [d], mode=EXTEND, scoring=sc, replay=True)
        assert rec7(res[0]) == rec7(pres[0]) and int(res["score"][0]) > 0
        assert cig.words(0).tolist() == pcig.words(0).tolist()
        assert int(pres["reserved"][0]) == 0 < int(res["reserved"][0])


@pytest.mark.gpu
def test_mixed_fates_in_one_batch(saln):
    """Case 4: fifteen pairs over five, the class-path pair among them; its
    record equals the class entry point's, steps included."""
    preconditions("mixed")
    five = xl.mixed_pairs()
    qs, ds = [p[0] for p in five], [p[1] for p in five]
    res, cig = check(saln, qs, ds, [(k % 5, k % 5) for k in range(15)], xl.MIXED_X, "cheap", 64)
    cres, ccig = saln.ends_free_align_batch([qs[3]], [ds[3]], mode=EXTEND, xdrop=xl.MIXED_X, scoring=elg.CHEAP)
    for k in (3, 8, 13):
        assert tuple(int(v) for v in res[k]) == tuple(int(v) for v in cres[0])
        assert cig.words(k).tolist() == ccig.words(0).tolist()


@pytest.mark.gpu
def test_a_window_after_a_run_that_wrote_every_row(saln):
    """Case 5.  In one context: the window pair with nothing pruned, so that
    every row of its area is written, then the same pair at X = 188 and 187,
    whose windows leave most of the area unwritten.  This does not prove that
    the tile fill reads no entry outside the windows (the allocator may hand
    out other memory for the later calls); it is cheap, and a read of a stale
    entry of the first run would show here."""
    preconditions("window")
    q, d = window_pair()
    X = model.no_drop(len(q), len(d), elg.scoring(None, "default")[1])
    with options(64):
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=X, replay=True)
    assert int(res["score"][0]) == 5162 and int(res["status"][0]) == 0 and len(cig[0]) >= 3
    for X in (188, 187):
        check(saln, [q], [d], [(0, 0)], X, "default", 64)


@pytest.mark.gpu
def test_the_budget_that_caps_the_codes_holds_the_replay(saln):
    """Case 6: 2,100 x 2,100 holds 2,217,600 bytes of codes and 689,840 of
    replay footprint (R = 1,024)."""
    preconditions("budget")
    q, d = budget_pair()
    TRACE_CAP = saln.ends_free.TRACE_CAP
    full, fcig = saln.xdrop_extend_long_batch([q], [d], xdrop=60)
    assert int(full["status"][0]) == 0 and int(full["score"][0]) > 5000 and len(fcig[0]) > 10
    res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, trace_budget=1_000_000)
    assert int(res["status"][0]) == TRACE_CAP and cig[0] == []                      # today's behaviour
    assert (int(res["q_begin"][0]), int(res["db_begin"][0])) == (-1, -1)
    assert (int(res["score"][0]), int(res["q_end"][0]), int(res["db_end"][0])) == \
        (int(full["score"][0]), int(full["q_end"][0]), int(full["db_end"][0]))
    with options(1024):
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, trace_budget=1_000_000, replay=True)
        assert int(res["status"][0]) == 0 and rec7(res[0]) == rec7(full[0])
        assert cig.words(0).tolist() == fcig.words(0).tolist()
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, trace_budget=600_000, replay=True)
        assert int(res["status"][0]) == TRACE_CAP and cig[0] == []
        assert (int(res["q_begin"][0]), int(res["db_begin"][0])) == (-1, -1)
        assert int(res["score"][0]) == int(full["score"][0])


@pytest.mark.gpu
def test_matrix(saln):
    """Case 7: the match / mismatch matrix gives the scalar replay's record and
    words; an asymmetric matrix matches the model under it."""
    q, d = window_pair()
    sm = saln.SubstitutionMatrix(b"ACGT", [[5 if a == b else -4 for b in range(4)] for a in range(4)], -8, -6)
    with options(64):
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=206, scoring=DEFAULT, replay=True)
        mres, mcig = saln.xdrop_extend_long_batch([q], [d], xdrop=206, scoring=sm, replay=True)
    assert tuple(int(v) for v in mres[0]) == tuple(int(v) for v in res[0]) and int(res["score"][0]) == 5162
    assert mcig.words(0).tolist() == cig.words(0).tolist()
    q, d = xl.diagonal_pair()
    asym = saln.SubstitutionMatrix(b"ACGT", ASYM, -5, -2)
    msc = efm.matrix_scoring(b"ACGT", ASYM, -5, -2)
    want, alive, L = model.align(q, d, 60, msc)
    windows = lm.schedule(q, d, 60, msc)[2]
    with options(64):
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=60, scoring=asym, replay=True)
    assert want.score > 0 and rec7(res[0]) == want.record()[:7]
    assert cig.words(0).tolist() == efm.cigar_words(want.cigar)
    assert 1 <= int(res["reserved"][0]) <= lm.steps_bound(windows)


@pytest.mark.gpu
def test_direction_left(saln):
    """Case 8."""
    q, d = xl.row0_pair()
    with options(64):
        r, c = saln.xdrop_extend_long(q, d, xdrop=xl.ROW0_X, scoring=elg.ROW0, replay=True)
        lr, lc = saln.xdrop_extend_long(q[::-1], d[::-1], xdrop=xl.ROW0_X, scoring=elg.ROW0, direction="left",
                                        replay=True)
    assert tuple(int(v) for v in r)[:6] == (468, 0, 0, 1330, 0, 300) and c == [(1030, "I"), (300, "=")]
    assert tuple(int(v) for v in lr)[:6] == (468, 0, 0, 1330, 0, 300) and lc == c[::-1]
    assert saln.xdrop_steps(lr) == saln.xdrop_steps(r) > 0


@pytest.mark.gpu
def test_score_only(saln):
    """Case 9: begins -1, no words, ends (and steps: the same fill) as without
    replay."""
    q, d = window_pair()
    with options(64):
        res, cig = saln.xdrop_extend_long_batch([q], [d], xdrop=206, cigar=False, replay=True)
    pres, pcig = saln.xdrop_extend_long_batch([q], [d], xdrop=206, cigar=False)
    assert tuple(int(v) for v in res[0]) == tuple(int(v) for v in pres[0]) == (5162, 0, -1, 1100, -1, 1070, 0,
                                                                               int(pres["reserved"][0]))
    assert cig[0] == [] and pcig[0] == []
