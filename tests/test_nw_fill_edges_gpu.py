"""GPU parity of the packed fills at the edges of their start-up and ramp
code: which bytes a lane reads of its query and its db rows, how the db rows
are staged, the steps before and after the steady loop, the sequences'
offsets in their buffers, and the table bodies' bail-out to the fallback
launch.  Every batch is compared with oracle.refcpu.check_pairs word for
word: score, end states, panic status, printed flag and CIGAR.

Plan order sorts a variant's pairs by db length, longest first, ties in batch
order, and a lane group takes two neighbours of that order (pair A, pair B);
16 pairs make a wave of 8 x 19 groups.  The batches below are laid out on
that."""
import numpy as np
import pytest

from nw_check import SCHEME, PlanRun, assert_batch, csr, rand_seq

pytestmark = pytest.mark.gpu

# query lengths at the lane edges of 8 x 19 groups (lanes of 19 columns, 152
# in a group), of 16 x 10 groups and of the wider ones
Q_LENS = [1, 2, 18, 19, 20, 37, 38, 39, 132, 133, 134, 151, 152, 153, 159, 160, 161, 256, 257, 512]
# db lengths round the row quads and lane shares of the staging, and 150
D_LENS = [1, 2, 7, 8, 9, 10, 11, 15, 16, 17, 31, 33, 150]

_cache: dict = {}


def _want(oracle, name, make):
    """(queries, dbs, oracle results) of batch `name`, built once."""
    if name not in _cache:
        queries, dbs = make()
        _cache[name] = (queries, dbs, oracle.check_pairs(*csr(queries), *csr(dbs), scoring=SCHEME))
    return _cache[name]


def _run(saln, queries, dbs, want, tag, *, steps=1, **kw):
    with PlanRun(saln, queries, dbs, SCHEME, **kw) as run:
        for step in range(steps):
            run.run()
            assert_batch(run.res, None if kw.get("score_only") else run.words, want, (tag, step),
                         score_only=bool(kw.get("score_only")))
        return [run.plan.pair_path(k) for k in range(len(queries))]


def _lane_edges(extra_db=()):
    """Every Q_LENS x D_LENS shape once.  A variant's 13 or fewer queries of
    one db length are neighbours in plan order, so a group's A and B differ
    in their query, and where the count per db length is odd also in their db.
    extra_db: one more pair per length given (a long db moves the whole
    launch of its variant to another frame)."""
    rng = np.random.default_rng(0xF111ED6E)
    shapes = [(lq, ld) for lq in Q_LENS for ld in D_LENS] + [(150, ld) for ld in extra_db] + \
             [(160, ld) for ld in extra_db]
    return [rand_seq(rng, lq) for lq, _ in shapes], [rand_seq(rng, ld) for _, ld in shapes]


# ------------------------------------------------------- lane and staging edges
@pytest.mark.parametrize("tab", [3, 2, 1, 0])
def test_lane_and_staging_edges(saln, oracle, saln_opt, tab):
    """nw.pk_tab: 3 row profiles (the default), 2 / 1 the table bodies at
    scale 4 / 2, 0 the generic body."""
    saln_opt("nw.pk_tab", tab)
    queries, dbs, want = _want(oracle, "lane", _lane_edges)
    paths = _run(saln, queries, dbs, want, ("lane edges", tab))
    packed = [p.packed for p in paths]
    assert all(packed), ("a pair left the packed fills", packed.index(False))
    if tab == 0:
        assert not any(p.table for p in paths)
    else:
        assert any(p.table for p in paths)


@pytest.mark.parametrize("kind", ["full", "score_only", "pipelined"])
def test_lane_edges_plan_kinds(saln, oracle, kind):
    queries, dbs, want = _want(oracle, "lane", _lane_edges)
    kw = {"full": {"full": True}, "score_only": {"score_only": True},
          "pipelined": {"pipelined": True}}[kind]
    _run(saln, queries, dbs, want, ("lane edges", kind), steps=2 if kind == "pipelined" else 1, **kw)


@pytest.mark.parametrize("ld_long", [600, 2528])
def test_lane_edges_rebasing_frame(saln, oracle, ld_long):
    """One long db per group width: its launch takes the rebasing frame, whose
    rows are staged as 16-bit words."""
    queries, dbs, want = _want(oracle, ("lane", ld_long), lambda: _lane_edges((ld_long,)))
    paths = _run(saln, queries, dbs, want, ("lane edges, long db", ld_long))
    print("rebasing:", sum(p.rebase for p in paths), "of", len(paths))
    assert any(p.rebase for p in paths)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33])
def test_pair_counts(saln, oracle, n):
    """Less than a wave, a whole wave, one pair more; odd counts leave a
    group without its B pair."""
    def make():
        rng = np.random.default_rng(100 + n)
        return ([rand_seq(rng, int(rng.integers(130, 153))) for _ in range(n)],
                [rand_seq(rng, int(rng.integers(140, 161))) for _ in range(n)])
    queries, dbs, want = _want(oracle, ("count", n), make)
    _run(saln, queries, dbs, want, ("pairs", n))
    _run(saln, queries, dbs, want, ("pairs, score only", n), score_only=True)


# ------------------------------------------------------------------------ ramp
def _ramp():
    """8 x 19 groups run steps 0-7 before their steady loop, 16 x 10 groups
    0-15; the loop takes two steps at a time while every lane is below the
    shorter db's last row.  So no steady step up to 10 (18) rows, one
    iteration at 11-12 (19-20), two at 13-14 (21-22)."""
    rng = np.random.default_rng(0x4A3F)
    shapes = []
    for lq in (150, 155):
        # equal db lengths in a group: four pairs of each
        shapes += [(lq, ld) for ld in range(1, 25) for _ in range(4)]
    # end cell in lane 0, 3 and 7, at its lane's first and last column, with
    # no, one and many steady steps
    shapes += [(lq, ld) for lq in (1, 19, 58, 76, 134, 152) for ld in (5, 5, 12, 12, 30, 30)]
    return [rand_seq(rng, lq) for lq, _ in shapes], [rand_seq(rng, ld) for _, ld in shapes]


def _ramp_by_one(first):
    """db lengths first, first - 1, .., 1, one pair each: every group's ldA
    and ldB differ by 1 (first even or odd: which of them is the longer's
    parity)."""
    def make():
        rng = np.random.default_rng(0x4A40 + first)
        shapes = [(lq, ld) for lq in (149, 158) for ld in range(first, 0, -1)]
        return [rand_seq(rng, lq) for lq, _ in shapes], [rand_seq(rng, ld) for _, ld in shapes]
    return make


def test_ramp_equal_db_lengths(saln, oracle):
    queries, dbs, want = _want(oracle, "ramp", _ramp)
    _run(saln, queries, dbs, want, "ramp")
    _run(saln, queries, dbs, want, "ramp, score only", score_only=True)


@pytest.mark.parametrize("first", [40, 41])
def test_ramp_db_lengths_differ_by_one(saln, oracle, first):
    queries, dbs, want = _want(oracle, ("ramp1", first), _ramp_by_one(first))
    _run(saln, queries, dbs, want, ("ramp by one", first))


# --------------------------------------------------------------------- offsets
BASE_SHAPES = [(150, 150), (152, 33), (19, 17), (37, 9), (1, 1), (160, 31), (133, 170)]


def _offsets():
    """Each base pair at q_off = s and db_off = 5 s + 3 (mod 16) for every s:
    a filler pair in front of it moves it there.  The first pair's query
    starts at byte 0 of its buffer and the last pair's db ends with its
    buffer (csr: no byte behind it)."""
    rng = np.random.default_rng(0x0FF5E7)
    base = [(rand_seq(rng, lq), rand_seq(rng, ld)) for lq, ld in BASE_SHAPES]
    queries, dbs = [base[0][0]], [base[0][1]]
    seen = set()
    for s in range(16):
        for q, d in base:
            qo, do = sum(map(len, queries)), sum(map(len, dbs))
            fq = (s - qo) % 16 or 16
            fd = (5 * s + 3 - do) % 16 or 16
            queries += [rand_seq(rng, fq), q]
            dbs += [rand_seq(rng, fd), d]
            seen.add(((qo + fq) % 16, (do + fd) % 16))
    assert {a for a, _ in seen} == set(range(16)) and {b for _, b in seen} == set(range(16))
    return queries, dbs


@pytest.mark.parametrize("kind", ["sync", "score_only"])
def test_offsets_mod_16(saln, oracle, kind):
    queries, dbs, want = _want(oracle, "offsets", _offsets)
    _run(saln, queries, dbs, want, ("offsets", kind), score_only=kind == "score_only")


# ------------------------------------------------------------------- bail path
BAD_BYTES = {"N": ord("N"), "a": ord("a"), "nul": 0x00, "ff": 0xFF}
# (sequence, index): a lane's first and last column, the query's last column;
# db row 1, the db's last row, and the edges of a row quad (3 | 4), of a
# lane's share (31 | 32) and of a staging batch (159 | 160)
BAIL_LQ, BAIL_LD = 150, 170
BAIL_SPOTS = [("q", 0), ("q", 18), ("q", 19), ("q", 37), ("q", 133), ("q", BAIL_LQ - 1),
              ("d", 0), ("d", BAIL_LD - 1), ("d", 3), ("d", 4), ("d", 31), ("d", 32),
              ("d", 159), ("d", 160)]


def _bail(byte):
    """Equal shapes, so plan order is batch order: pairs 16 w .. 16 w + 15
    are wave w, an even pair is its group's A.  Every (spot, A or B) has a
    wave of its own with the byte in one pair, and a clean wave behind it."""
    def make():
        rng = np.random.default_rng(0xBA11)
        n = 32 * 2 * len(BAIL_SPOTS)
        queries = [bytearray(rand_seq(rng, BAIL_LQ)) for _ in range(n)]
        dbs = [bytearray(rand_seq(rng, BAIL_LD)) for _ in range(n)]
        for c, (side, at) in enumerate(BAIL_SPOTS):
            for half in range(2):  # in A only, in B only
                pair = 32 * (2 * c + half) + 6 + half
                (queries if side == "q" else dbs)[pair][at] = byte
        return [bytes(q) for q in queries], [bytes(d) for d in dbs]
    return make


@pytest.mark.parametrize("pipelined", [False, True], ids=["sync", "async"])
@pytest.mark.parametrize("byte", list(BAD_BYTES))
def test_bail_to_fallback(saln, oracle, byte, pipelined):
    """One byte that is not A, C, G or T sends its wave to the fallback
    launch; the async plan runs that launch on its walk stream."""
    queries, dbs, want = _want(oracle, ("bail", byte), _bail(BAD_BYTES[byte]))
    _run(saln, queries, dbs, want, ("bail", byte, pipelined), pipelined=pipelined,
         steps=2 if pipelined else 1)
