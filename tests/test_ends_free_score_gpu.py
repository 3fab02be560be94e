"""GPU: the score-only search (saln_ends_free_score_*, ends_free_score_kernels.hip)
against the plain model tests/ends_free_model.py and against the `score` field
of ends_free_align_batch(..., cigar=False), the i32 fill this engine already
had.  The packed-i16 fill holds two pairs per lane group: the cases below aim
at what that can get wrong (unequal halves, a ghost row past the shorter db, a
group with one pair, empty sequences beside real ones, the int16 guard's
edges)."""
import random

import numpy as np
import pytest

import ends_free_model as model

pytestmark = pytest.mark.gpu

LOCAL, SEMI, OVERLAP, EXTEND = model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP, model.EXTEND
SCALAR = (5, -4, -8, -6)
ALPHABET = b"ACGT"
TABLE = [[6, -3, -1, -4], [-3, 7, -5, -2], [-1, -5, 5, -3], [-4, -2, -3, 8]]   # not symmetric on purpose
TABLE[0][2], TABLE[3][1] = 2, -6
SENTINEL = -123456789


def rand_seq(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def related(rng, q, m, letters=b"ACGT"):
    """A db of m bytes that shares stretches with q, so that scores are not all tiny."""
    out = bytearray()
    while len(out) < m:
        if q and rng.random() < 0.6:
            a = rng.randrange(len(q))
            out += q[a:a + rng.randint(1, 40)]
        else:
            out += rand_seq(rng, rng.randint(1, 10), letters)
        if rng.random() < 0.3 and out:
            out[rng.randrange(len(out))] = rng.choice(letters)
    return bytes(out[:m])


def scorings(saln):
    return {"scalar": (SCALAR, SCALAR),
            "matrix": (saln.SubstitutionMatrix(ALPHABET, TABLE, -7, -2),
                       model.matrix_scoring(ALPHABET, TABLE, -7, -2))}


def expect(q, d, mode, mscoring):
    return model.linear_ends(q, d, mode, mscoring)[0]


def run_plan(saln, qs, ds, pairs, mode, scoring, runs=1):
    """The plan's scores (one array per execute), its info(), and the sentinel
    slot behind the scores after each execute."""
    import torch
    qb, qo = saln.pack_csr(qs)
    db, do = saln.pack_csr(ds)
    plan = saln.EndsFreeScorePlan(qo, do, pairs, mode=mode, scoring=scoring)
    dq = torch.from_numpy(np.concatenate([qb, np.zeros(16, np.uint8)])).cuda()
    dd = torch.from_numpy(np.concatenate([db, np.zeros(16, np.uint8)])).cuda()
    outs = [torch.full((plan.n_pairs + 1,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(runs)]
    for o in outs:
        plan.execute(dq, dd, o)
    torch.cuda.synchronize()
    info = plan.info()
    n = plan.n_pairs
    plan.close()
    got = [o.cpu().numpy() for o in outs]
    return [g[:n] for g in got], info, [int(g[n]) for g in got]


def i32_scores(saln, qs, ds, pairs, mode, scoring):
    res, _ = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=scoring, cigar=False)
    return res["score"].astype(np.int32)


# ------------------------------------------------ 1. every class, mode and scoring
CLASS_QUERIES = {0: (1, 7, 160), 1: (161, 200, 256), 2: (257, 400, 512), 3: (513, 700, 1024)}


@pytest.fixture(scope="module")
def class_batches():
    """Per class: (queries, dbs, scrambled pair list): 9 pairs, query lengths at
    both ends of the class, db lengths from 1 to about 300."""
    out = {}
    for cls, lens in CLASS_QUERIES.items():
        rng = random.Random(0x5C0 + cls)
        qs = [rand_seq(rng, n) for n in lens]
        ds = [related(rng, qs[k % 3], m) for k, m in enumerate((1, 2, 17, 64, 65, 130, 233, 299, 300))]
        pairs = [(k % 3, k) for k in range(9)]
        rng.shuffle(pairs)
        out[cls] = (qs, ds, pairs)
    return out


@pytest.mark.parametrize("kind", ("scalar", "matrix"))
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
@pytest.mark.parametrize("cls", (0, 1, 2, 3))
def test_every_class_mode_and_scoring(saln, class_batches, cls, mode, kind):
    qs, ds, pairs = class_batches[cls]
    scoring, mscoring = scorings(saln)[kind]
    lanes_cols = {0: (16, 10), 1: (16, 16), 2: (64, 8), 3: (64, 16)}[cls]
    assert all(saln.ends_free.pair_geometry(len(q)) == lanes_cols for q in qs)
    assert all(saln.ends_free.score_path(len(qs[a]), len(ds[b]), mode, scoring) for a, b in pairs)
    got = saln.ends_free.score_batch(qs, ds, pairs, mode=mode, scoring=scoring)
    want = [expect(qs[a], ds[b], mode, mscoring) for a, b in pairs]
    assert got.dtype == np.int32 and got.tolist() == want


# ------------------------------------------------------------ 2. unequal halves
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
@pytest.mark.parametrize("kind", ("scalar", "matrix"))
def test_unequal_halves(saln, mode, kind):
    rng = random.Random(77)
    scoring, mscoring = scorings(saln)[kind]
    short_q, long_q = rand_seq(rng, 9), rand_seq(rng, 155)
    long_d, short_d = related(rng, short_q, 120), related(rng, long_q, 70)   # one power-of-two bucket
    qs, ds = [short_q, long_q], [long_d, short_d]
    want = [expect(short_q, long_d, mode, mscoring), expect(long_q, short_d, mode, mscoring)]
    for order in ([(0, 0), (1, 1)], [(1, 1), (0, 0)]):
        got, info, _ = run_plan(saln, qs, ds, order, mode, scoring)
        assert info == (2, 0)
        assert got[0].tolist() == [want[a] for a, _ in order]
    for k in (0, 1):
        assert saln.ends_free.score_batch(qs, ds, [(k, k)], mode=mode, scoring=scoring).tolist() == [want[k]]


# ---------------------------------------------------------------- 3. the ghost row
def test_the_ghost_row(saln):
    """AAAAAAAC against AAAAAAA, semi-global under (5, -4, -10, -1): the query
    has one column more than the db has rows, so an insertion is forced: seven
    matches and the C inserted, 35 - 11 = 24.  A kernel that counted one ghost
    row past the db, holding the partner's A, would find eight rows: seven
    matches and C against A, 35 - 4 = 31.  Dbs of fewer than 64 rows share a
    launch, so the two pairs below share a group; of a group's pairs the earlier
    in pair order is the low half."""
    scoring = (5, -4, -10, -1)
    q, d = b"AAAAAAAC", b"AAAAAAA"
    assert expect(q, d, SEMI, scoring) == 24
    assert expect(q, d + b"A", SEMI, scoring) == 31
    partner_q, partner_d = b"ACGTACGTAC", b"A" * 40
    want_p = expect(partner_q, partner_d, SEMI, scoring)
    ef = saln.ends_free
    assert ef.score_path(len(q), len(d), SEMI, scoring) and ef.score_path(len(partner_q), 40, SEMI, scoring)
    qs, ds = [q, partner_q], [d, partner_d]
    for order in ([(0, 0), (1, 1)], [(1, 1), (0, 0)]):       # the low half, then the high half
        got, info, tail = run_plan(saln, qs, ds, order, SEMI, scoring)
        assert info == (2, 0) and tail == [SENTINEL]
        assert got[0].tolist() == [24 if a == 0 else want_p for a, _ in order]
    # local under the same pairing: its ghost rows must not count either
    for order in ([(0, 0), (1, 1)], [(1, 1), (0, 0)]):
        got, _, _ = run_plan(saln, qs, ds, order, LOCAL, scoring)
        assert got[0].tolist() == [expect(qs[a], ds[a], LOCAL, scoring) for a, _ in order] and 35 in got[0]


# ----------------------------------------- 4. partly filled groups, waves, workgroups
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
@pytest.mark.parametrize("lanes,count", [(16, 1), (16, 2), (16, 3), (16, 7), (16, 9), (16, 70),
                                         (64, 1), (64, 2), (64, 3), (64, 5)])
def test_partly_filled_groups(saln, mode, lanes, count):
    rng = random.Random(1000 * lanes + count)
    lo, hi = (20, 150) if lanes == 16 else (260, 330)
    qs = [rand_seq(rng, rng.randint(lo, hi)) for _ in range(count)]
    ds = [related(rng, qs[k], rng.randint(33, 63)) for k in range(count)]    # one launch
    assert all(saln.ends_free.pair_geometry(len(q))[0] == lanes for q in qs)
    pairs = [(k, k) for k in range(count)]
    got, info, tail = run_plan(saln, qs, ds, pairs, mode, SCALAR)
    assert info == (count, 0) and tail == [SENTINEL]
    assert got[0].tolist() == [expect(qs[k], ds[k], mode, SCALAR) for k in range(count)]


# ------------------------------------------------------------ 5. empty sequences
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
@pytest.mark.parametrize("kind", ("scalar", "matrix"))
def test_empty_sequences_beside_real_ones(saln, mode, kind):
    rng = random.Random(5)
    scoring, mscoring = scorings(saln)[kind]
    q, d = rand_seq(rng, 30), rand_seq(rng, 25)
    qs, ds = [q, b""], [d, b""]
    o, e = (SCALAR[2], SCALAR[3]) if kind == "scalar" else (-7, -2)
    for other in ((1, 0), (0, 1), (1, 1)):                     # n = 0, m = 0, both
        for pairs in ([(0, 0), other], [other, (0, 0)], [other], [other, other, (0, 0)]):
            got, info, tail = run_plan(saln, qs, ds, pairs, mode, scoring)
            assert info == (len(pairs), 0) and tail == [SENTINEL]
            want = [expect(qs[a], ds[b], mode, mscoring) for a, b in pairs]
            assert got[0].tolist() == want
            assert got[0].tolist() == i32_scores(saln, qs, ds, pairs, mode, scoring).tolist()
    assert expect(q, b"", SEMI, mscoring) == o + 30 * e and expect(b"", d, SEMI, mscoring) == 0


# ------------------------------------------------------------ 6. the guard's edges
def test_local_guard_edge_on_the_device(saln):
    q = b"G" * 1024
    for match, packed in ((31, True), (32, False)):
        scoring = (match, -31, -31, -31)
        got, info, _ = run_plan(saln, [q], [q], [(0, 0)], LOCAL, scoring)
        assert got[0].tolist() == [1024 * match] == [expect(q, q, LOCAL, scoring)]
        assert info == ((1, 0) if packed else (0, 1))


def test_semi_global_guard_edge_on_the_device(saln):
    """A = 32; 1,019 and 1,020 columns of one base against 64 rows of another:
    nothing matches and the values go down to about -(n + 4) A."""
    scoring = (5, -4, -32, -6)
    for n, packed in ((1019, True), (1020, False)):
        q, d = b"A" * n, b"C" * 64
        got, info, _ = run_plan(saln, [q], [d], [(0, 0)], SEMI, scoring)
        assert got[0].tolist() == [expect(q, d, SEMI, scoring)]
        assert info == ((1, 0) if packed else (0, 1))
    # the same depth with gaps that cost their full A at every step
    scoring = (1, -1, 0, -32)
    for n, packed in ((1019, True), (1020, False)):
        q, d = b"A" * n, b"C" * 64
        got, info, _ = run_plan(saln, [q], [d], [(0, 0)], SEMI, scoring)
        assert got[0].tolist() == [expect(q, d, SEMI, scoring)]
        assert info == ((1, 0) if packed else (0, 1))


# ------------------------------------------------------------- 7. the longest db
def test_the_longest_db(saln):
    rng = random.Random(65000)
    q = rand_seq(rng, 40)
    d = bytearray(rand_seq(rng, 65000))
    d[64000:64040] = q                                  # the hit sits near the end
    d = bytes(d)
    ef = saln.ends_free
    assert ef.score_path(40, 65000, LOCAL, SCALAR)
    assert ef.score_geometry(40, 65000) == (1, 2 * (65000 + 32))
    got, info, tail = run_plan(saln, [q], [d], [(0, 0)], LOCAL, SCALAR)
    assert info == (1, 0) and tail == [SENTINEL]
    assert got[0].tolist() == i32_scores(saln, [q], [d], [(0, 0)], LOCAL, SCALAR).tolist() == [200]


# ------------------------------------------------------------ 8. overlap and extend
@pytest.mark.parametrize("mode", (OVERLAP, EXTEND))
@pytest.mark.parametrize("kind", ("scalar", "matrix"))
def test_overlap_and_extend_run_the_i32_fill(saln, mode, kind):
    rng = random.Random(8 + mode)
    scoring, mscoring = scorings(saln)[kind]
    qs = [rand_seq(rng, n) for n in (0, 5, 90, 300)]
    ds = [qs[2][40:] + rand_seq(rng, 30), qs[3][:120], rand_seq(rng, 9), b""]
    pairs = [(3, 1), (0, 0), (2, 0), (1, 2), (2, 3), (3, 0), (1, 1)]
    got, info, tail = run_plan(saln, qs, ds, pairs, mode, scoring)
    assert info == (0, len(pairs)) and tail == [SENTINEL]
    assert got[0].tolist() == [expect(qs[a], ds[b], mode, mscoring) for a, b in pairs]


# ------------------------------------------------------- 9. ends_free.score_i16 = 0
@pytest.mark.parametrize("kind", ("scalar", "matrix"))
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
def test_score_i16_off(saln, saln_opt, class_batches, mode, kind):
    scoring, _ = scorings(saln)[kind]
    for cls in (0, 3):
        qs, ds, pairs = class_batches[cls]
        on, info_on, _ = run_plan(saln, qs, ds, pairs, mode, scoring)
        saln_opt("ends_free.score_i16", 0)
        off, info_off, _ = run_plan(saln, qs, ds, pairs, mode, scoring)
        saln_opt("ends_free.score_i16", 1)
        assert info_on == (9, 0) and info_off == (0, 9)
        assert on[0].tolist() == off[0].tolist()


# ------------------------------------------------------------------ 10. plan reuse
@pytest.mark.parametrize("mode", (LOCAL, SEMI, OVERLAP))
def test_plan_reuse(saln, class_batches, mode):
    qs, ds, pairs = class_batches[1]
    got, _, tail = run_plan(saln, qs, ds, pairs, mode, SCALAR, runs=2)
    assert tail == [SENTINEL, SENTINEL]
    assert got[0].tolist() == got[1].tolist()
    assert got[0].tolist() == saln.ends_free.score_batch(qs, ds, pairs, mode=mode, scoring=SCALAR).tolist()


# ------------------------------------------------------------------ 11. all-vs-all
@pytest.mark.parametrize("mode", (LOCAL, SEMI, EXTEND))
def test_all_vs_all_db_outer(saln, mode):
    rng = random.Random(11)
    qs = [rand_seq(rng, n) for n in (12, 170, 33)]
    ds = [related(rng, qs[k % 3], m) for k, m in enumerate((50, 7, 120, 64))]
    got = saln.ends_free.score_batch(qs, ds, None, mode=mode)
    assert got.tolist() == [expect(q, d, mode, SCALAR) for d in ds for q in qs]


# ---------------------------------------------------------------------- 12. random
@pytest.mark.parametrize("mode", (LOCAL, SEMI))
@pytest.mark.parametrize("kind", ("scalar", "matrix"))
def test_random(saln, mode, kind):
    rng = random.Random(1200 + mode + (7 if kind == "matrix" else 0))
    if kind == "scalar":
        # inside the engine's domain, with parameters of every size the guard lets 200 x 200 keep packed
        ma = rng.randint(1, 60)
        scoring = mscoring = (ma, -rng.randint(1, 60), -rng.randint(0, 60), -rng.randint(1, 60))
    else:
        scoring, mscoring = scorings(saln)["matrix"]
    qs = [rand_seq(rng, rng.randint(1, 200)) for _ in range(200)]
    ds = [related(rng, qs[k], rng.randint(1, 200)) for k in range(200)]
    pairs = [(k, k) for k in range(200)]
    rng.shuffle(pairs)
    got, info, tail = run_plan(saln, qs, ds, pairs, mode, scoring)
    assert info == (200, 0) and tail == [SENTINEL]
    assert got[0].tolist() == i32_scores(saln, qs, ds, pairs, mode, scoring).tolist()
    for k in rng.sample(range(200), 24):
        a, b = pairs[k]
        assert int(got[0][k]) == expect(qs[a], ds[b], mode, mscoring), k
