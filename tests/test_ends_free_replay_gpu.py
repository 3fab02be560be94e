"""GPU: the tiled replay traceback of the ends-free engine
(saln_ends_free_replay_align_batch, ends_free_replay_kernels.hip), local,
semi-global and overlap.  Every comparison is exact on the whole record and
every word, against two references: the long entry point with its default
budget (the full trace, GPU against GPU) and, wherever the db has at most 200
rows (or the query 5 columns), the plain model.  The inputs and their
preconditions (which tile edge a path crosses, and how) are in
test_ends_free_replay.py (no device); a tile there is 1,024 columns x 64 rows,
set here through the option ends_free.tile_rows."""
import numpy as np
import pytest

import test_ends_free_long_gpu as lg
import test_ends_free_replay as cpu
import test_overlap_gpu as og

pytestmark = pytest.mark.gpu

LOCAL, SEMI, OVERLAP = cpu.LOCAL, cpu.SEMI, cpu.OVERLAP
MODES = cpu.MODES
SCHEMES = lg.SCHEMES
TRACE_CAP = 8
MODEL_ROWS = 200


def _expect(q, d, mode, scheme=None):
    """(record, words) of the mode's plain model; the runs are shared with the
    other ends-free GPU files."""
    return og._expect(q, d, scheme) if mode == OVERLAP else lg._expect(q, d, mode, scheme)


def _plist(qs, ds, pairs):
    return pairs if pairs is not None else [(a, b) for b in range(len(ds)) for a in range(len(qs))]


def _same(res, cig, ref, rcig):
    assert len(res) == len(ref) and (res == ref).all(), np.nonzero(res != ref)[0][:8]
    for k in range(len(res)):
        assert cig.words(k).tolist() == rcig.words(k).tolist(), k


def _check(saln, qs, ds, pairs, mode, scheme=None, tile_rows=64, model=None, **kw):
    """One batch through the replay entry point at tile_rows, compared with the
    long entry point under its default budget and with the model (model=None:
    wherever the db has at most MODEL_ROWS rows)."""
    from sequencealigning_amd import _lib
    with _lib.options(**{"ends_free.tile_rows": tile_rows}):
        res, cig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=scheme, replay=True, **kw)
    ref, rcig = saln.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=scheme)
    plist = _plist(qs, ds, pairs)
    assert len(res) == len(cig) == len(plist)
    _same(res, cig, ref, rcig)
    for k, (a, b) in enumerate(plist):
        if model is False or (model is None and len(ds[b]) > MODEL_ROWS):
            continue
        rec, words = _expect(qs[a], ds[b], mode, scheme)
        assert tuple(int(v) for v in res[k]) == rec, (k, len(qs[a]), len(ds[b]))
        assert cig.words(k).tolist() == words, (k, len(qs[a]), len(ds[b]))
    return res, cig


# ------------------------------------------------------------------ 1. the edge batch
@pytest.fixture(scope="module")
def edge_batch():
    qs, ds = lg._make_edge_batch()
    rng = np.random.default_rng(0x7113ED6E)
    q = qs[7]
    for m in (63, 64, 65, 127, 128, 129, 200):   # windows over column 1,024, of the row-block edges' sizes
        lo = 1024 - m // 2
        ds.append((lg._mutated(rng, q[lo:lo + m + 4]) + lg._rand(rng, 8))[:m])
        assert len(ds[-1]) == m
    return qs, ds


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("mode", MODES)
def test_edge_batch(saln, edge_batch, mode, scheme):
    qs, ds = edge_batch
    res, _ = _check(saln, qs, ds, None, mode, scheme)
    assert (res["status"] == 0).all()


# ------------------------------------------------------------------ 2. the corner
@pytest.mark.parametrize("mode", MODES)
def test_corner(saln, mode):
    q, d = cpu.corner_pair()
    res, cig = _check(saln, [q], [d], [(0, 0)], mode)
    if mode != SEMI:
        assert cig[0] == [(128, "=")]
        assert tuple(int(res[0][f]) for f in ("q_begin", "q_end", "db_begin", "db_end")) == (960, 1088, 0, 128)
    else:
        assert cig[0] == [(960, "I"), (128, "="), (112, "I")]


# ------------------------------------------------------------------ 3. gaps over the edges
@pytest.mark.parametrize("mode", MODES)
def test_gaps_over_the_edges(saln, mode):
    q, d = cpu.cpu.insertion_pair()
    _, cig = _check(saln, [q], [d], [(0, 0)], mode, model=True)
    assert cpu.cpu.covers(cig[0], "I", 1024)
    q, d = cpu.deletion_pair()
    res, cig = _check(saln, [q], [d], [(0, 0)], mode)
    i = int(res["db_begin"][0])
    runs = []
    for n, op in cig[0]:
        if op == "D":
            runs.append((i + 1, i + n))
        i += n if op in "=XD" else 0
    assert any(lo <= 64 < hi for lo, hi in runs), cig[0]   # a D run steps from row 65 to row 64


# ------------------------------------------------------------------ 4. begins and ends on tile edges
def test_begin_and_end_on_tile_edges(saln):
    q, d = cpu.begin_on_edges_pair()
    res, _ = _check(saln, [q], [d], [(0, 0)], LOCAL)
    assert (int(res["q_begin"][0]), int(res["db_begin"][0])) == (1024, 64)
    for db_end in (64, 65):
        q, d = cpu.end_on_edges_pair(db_end)
        res, _ = _check(saln, [q], [d], [(0, 0)], LOCAL)
        assert (int(res["db_end"][0]), int(res["q_end"][0])) == (db_end, 1064)


# ------------------------------------------------------------------ 5., 6. the borders
def test_semi_global_reaches_row_0_above_column_1024(saln):
    q, d = cpu.row0_insertion_pair()
    _, cig = _check(saln, [q], [d], [(0, 0)], SEMI)
    assert cig[0] == [(1050, "I"), (100, "=")]


def test_overlap_stops_on_the_borders(saln):
    q, d = cpu.overlap_row0_pair()
    res, _ = _check(saln, [q], [d], [(0, 0)], OVERLAP)
    assert (int(res["q_begin"][0]), int(res["db_begin"][0])) == (1200, 0)
    q, d = cpu.overlap_col0_pair()
    res, _ = _check(saln, [q], [d], [(0, 0)], OVERLAP)
    assert (int(res["q_begin"][0]), int(res["db_begin"][0])) == (0, 100)
    # both in one batch with the pairs that give no alignment at all
    qs = [q, cpu.overlap_row0_pair()[0], b"N" * 1100, b""]
    ds = [d, cpu.overlap_row0_pair()[1], b"R" * 70]
    _check(saln, qs, ds, None, OVERLAP)


# ------------------------------------------------------------------ 7. one chunk, many row blocks
@pytest.mark.parametrize("mode", MODES)
def test_one_chunk_pair(saln, mode):
    from sequencealigning_amd import _lib
    rng = np.random.default_rng(0x1C5)
    q = b"ACGTA"
    d = lg._rand(rng, 30000) + q + lg._rand(rng, 65001 - 30005)
    R = _lib.get_option("ends_free.tile_rows")[0]
    assert saln.ends_free.pair_path_long(5, 65001) == (1, 1)
    assert saln.ends_free.replay_bytes(5, 65001) == sum(cpu.components(5, 65001, R))
    assert cpu.components(5, 65001, R)[0] == 0                      # no kept column
    _check(saln, [q], [d], [(0, 0)], mode, tile_rows=R, model=True)


# ------------------------------------------------------------------ 8. the default R, no model
@pytest.mark.parametrize("mode", MODES)
def test_default_tile_rows(saln, mode):
    from sequencealigning_amd import _lib
    rng = np.random.default_rng(0xDEFA + mode)
    qs = [lg._rand(rng, 2100) for _ in range(3)]
    ds = []
    for q in qs:
        a = lg._mutated(rng, q[:1050]) + lg._mutated(rng, q[1050:])
        ds.append((a + lg._rand(rng, 30))[:2100])
    assert all(len(d) == 2100 for d in ds)
    pairs = [(k, k) for k in range(3)]
    R = _lib.get_option("ends_free.tile_rows")[0]
    res, cig = _check(saln, qs, ds, pairs, mode, tile_rows=R, model=False)
    for k in range(3):
        r, c = res[k], cig[k]
        assert int(r["status"]) == 0 and int(r["score"]) > 2100 * 2 and len(c) == int(r["cigar_len"])
        assert saln.ends_free.cigar_score(c) == int(r["score"])
        assert sum(n for n, op in c if op in "=XI") == int(r["q_end"]) - int(r["q_begin"])
        assert sum(n for n, op in c if op in "=XD") == int(r["db_end"]) - int(r["db_begin"])


# ------------------------------------------------------------------ 9. the budget
@pytest.mark.parametrize("mode", MODES)
def test_budget(saln, mode):
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    qs, ds = cpu.budget_pairs()
    pairs = [(k, k) for k in range(6)]
    small, full = ef.replay_bytes(3000, 200, 64), ef.trace_bytes_long(3000, 200)
    budget = (small + full) // 2
    assert small < budget < full
    with _lib.options(**{"ends_free.tile_rows": 64}):
        # one pair: the full trace does not fit the budget, the replay does
        res, cig = ef.ends_free_align_long_batch(qs[:1], ds[:1], mode=mode, trace_budget=budget)
        rec, words = _expect(qs[0], ds[0], mode)
        assert tuple(int(v) for v in res[0]) == lg._score_only(rec, TRACE_CAP) and cig[0] == []
        res, cig = ef.ends_free_align_long_batch(qs[:1], ds[:1], mode=mode, trace_budget=budget, replay=True)
        assert tuple(int(v) for v in res[0]) == rec and cig.words(0).tolist() == words
        # below the replay's footprint: both give the score-only record
        for replay in (False, True):
            res, cig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, trace_budget=small - 1,
                                                     replay=replay)
            for k in range(6):
                rec, _ = _expect(qs[k], ds[k], mode)
                assert tuple(int(v) for v in res[k]) == lg._score_only(rec, TRACE_CAP) and cig[k] == [], k
        # one pair at a time fits: the same records, the words contiguous in pair order
        one, ocig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, replay=True)
        res, cig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, trace_budget=small + 8, replay=True)
    _same(res, cig, one, ocig)
    for k in range(6):
        rec, words = _expect(qs[k], ds[k], mode)
        assert tuple(int(v) for v in res[k]) == rec and cig.words(k).tolist() == words, k


# ------------------------------------------------------------------ 10. the mixed batch
@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch(saln, mode):
    qs, ds, pairs = lg._make_mixed_batch()
    pairs = pairs + [(3, 3), (1, 1), (0, 0), (3, 3)]       # repeated pairs, long and short
    path = [saln.ends_free.pair_path_long(len(qs[a]), len(ds[b]))[0] for a, b in pairs]
    assert path == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1]
    res, cig = _check(saln, qs, ds, pairs, mode, model=False)
    assert res[3] == res[13] == res[16] and cig[3] == cig[13] == cig[16] != []
    assert sum(cig.words(k).size for k in range(len(pairs))) == int(res["cigar_len"].sum())


# ------------------------------------------------------------------ 11. the option
@pytest.mark.parametrize("mode", MODES)
def test_every_tile_rows_gives_the_same(saln, mode):
    from sequencealigning_amd import _lib
    rng = np.random.default_rng(0x711E + mode)
    qs = [lg._rand(rng, n) for n in (1500, 2049, 1100)]
    ds = [(lg._mutated(rng, qs[0][200:1480]) + lg._rand(rng, 20))[:1290],       # more rows than the largest tile
          lg._mutated(rng, qs[1][900:1200]),
          lg._rand(rng, 90) + qs[2][1000:1100]]
    assert len(ds[0]) == 1290
    ref = None
    for R in cpu.TILE_ROWS:
        out = _check(saln, qs, ds, None, mode, tile_rows=R, model=False)
        if ref is not None:
            _same(out[0], out[1], ref[0], ref[1])
        ref = out
    # any other value: the replay batch is refused, the other entry points run
    with _lib.options(**{"ends_free.tile_rows": 100}):
        msg = lg._refused(lambda: saln.ends_free_align_long_batch(qs, ds, mode=mode, replay=True))
        assert "tile_rows" in msg and "100" in msg
        lg._refused(lambda: saln.ends_free_align_long_batch(qs, ds, mode=mode, replay=True, cigar=False))
        res, cig = saln.ends_free_align_long_batch(qs, ds, mode=mode)
        _same(res, cig, ref[0], ref[1])
        short, _ = saln.ends_free_align_batch([qs[0][:300]], [ds[1]], mode=mode)
        assert int(short["status"][0]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_score_only_equals_the_long_entry_point(saln, edge_batch, mode):
    qs, ds = edge_batch
    a, acig = saln.ends_free_align_long_batch(qs, ds, mode=mode, cigar=False, replay=True)
    b, bcig = saln.ends_free_align_long_batch(qs, ds, mode=mode, cigar=False)
    assert (a == b).all() and int(a["cigar_len"].sum()) == 0 and (a["q_begin"] == -1).all()
    assert all(acig[k] == [] for k in range(len(a)))


def test_one_pair_forms(saln):
    q, d = cpu.corner_pair()
    for fn in (saln.local_align_long, saln.overlap_align_long):
        rec, cigar = fn(q, d, replay=True)
        assert cigar == [(128, "=")] and tuple(int(v) for v in rec) == tuple(int(v) for v in fn(q, d)[0])
    rec, cigar = saln.semi_global_align_long(q, d, replay=True)
    assert cigar == [(960, "I"), (128, "="), (112, "I")]
