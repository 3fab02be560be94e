"""GPU: the ends-free engine's extension mode, SALN_MODE_EXTEND (the kMode ==
SALN_MODE_EXTEND instances of ends_free_kernels.hip): pinned at the origin,
free at its end.  Every comparison is exact against the plain model
(ends_free_model.py): the whole result record and the CIGAR, word for word, with
CIGAR, score only and through EndsFreePlan; alignment_score of every returned
alignment is its score."""
import random

import numpy as np
import pytest

import ends_free_model as model

EXTEND = model.EXTEND
DEFAULT = (5, -4, -8, -6)
OPEN0 = (5, -4, 0, -3)            # gap_open = 0
# 24 symbols, random asymmetric entries in -8 .. 11.
ALPHABET24 = b"ARNDCQEGHILKMFPSTWYVBZXU"
_rng24 = random.Random(0x24E8)
TABLE24 = [[_rng24.randint(-8, 11) for _ in range(24)] for _ in range(24)]
GAPS24 = (-10, -2)
assert any(TABLE24[a][b] != TABLE24[b][a] for a in range(24) for b in range(24))
assert min(min(r) for r in TABLE24) == -8 and max(max(r) for r in TABLE24) == 11
SCORINGS = ["default", "open0", "m24"]


def scoring(saln, name):
    """(the engine's scoring argument, the model's Scoring, the bytes sequences draw from)."""
    if name == "m24":
        return (saln.SubstitutionMatrix(ALPHABET24, TABLE24, *GAPS24),
                model.matrix_scoring(ALPHABET24, TABLE24, *GAPS24), ALPHABET24 + b"O")
    scheme = DEFAULT if name == "default" else OPEN0
    return scheme, model.scalar_scoring(*scheme), b"ACGT"


def rand_seq(rng, n, letters):
    return bytes(rng.choice(letters) for _ in range(n))


def anchored(rng, q, length, letters):
    """`length` bytes: a mutated copy of a prefix of q (8 % substitutions, a few
    indels) from the first byte on, then a random tail."""
    keep = rng.randint((length + 1) // 2, length)
    out, i = bytearray(), 0
    while len(out) < keep and i < len(q):
        u = rng.random()
        if u < 0.08:
            out.append(rng.choice(letters))
            i += 1
        elif u < 0.095:
            i += rng.randint(1, 3)                            # deletion
        elif u < 0.11:
            out += rand_seq(rng, rng.randint(1, 3), letters)  # insertion
        else:
            out.append(q[i])
            i += 1
    out = out[:length]
    return bytes(out) + rand_seq(rng, length - len(out), letters)


def expect(q, d, msc, walk=True):
    a = model.align(q, d, EXTEND, msc, walk=walk)
    return a.record(), model.cigar_words(a.cigar)


def compare(saln, qs, ds, pairs, sc, msc, batch=None, **kw):
    """Runs one batch in extension mode and compares every pair with the model
    and with alignment_score."""
    batch = batch or saln.ends_free_align_batch
    res, cig = batch(qs, ds, pairs, mode=EXTEND, scoring=sc, **kw)
    assert len(res) == len(cig) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        rec, words = expect(qs[a], ds[b], msc)
        assert tuple(int(v) for v in res[k]) == rec, (k, len(qs[a]), len(ds[b]), qs[a][:40], ds[b][:40])
        assert cig.words(k).tolist() == words, (k, qs[a][:40], ds[b][:40])
        assert (rec[2], rec[4]) == (0, 0)
        assert saln.alignment_score(qs[a], ds[b], (res[k], cig[k]), sc) == int(res["score"][k]), k
    return res, cig


# ------------------------------------------------------------------ 1. class edges
EDGE_QUERIES = (1, 9, 10, 11, 160, 161, 256, 257, 512, 513, 1024)
EDGE_DBS = (1, 2, 15, 16, 17, 63, 64, 65, 90)


def edge_batch(letters, seed):
    """Every class, pad columns in each (9, 11, 161, 257, 513 are no multiple
    of their class's columns per lane) and full last lanes (10, 160, 256, 512,
    1024); dbs of 1 to 90 rows, each a mutated copy of the query's prefix plus
    a random tail, and the empty sequences."""
    rng = random.Random(seed)
    qs = [rand_seq(rng, n, letters) for n in EDGE_QUERIES]
    ds, pairs = [], []
    for a, q in enumerate(qs):
        for m in EDGE_DBS:
            pairs.append((a, len(ds)))
            ds.append(anchored(rng, q, m, letters))
    qs.append(b"")
    ds.append(b"")
    pairs += [(len(qs) - 1, 0), (0, len(ds) - 1), (len(qs) - 1, len(ds) - 1), (4, len(ds) - 1)]   # n = 0, m = 0
    return qs, ds, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_class_edges(saln, name):
    """The accepted call: the parent refuses mode 8 with SALN_E_INVALID."""
    sc, msc, letters = scoring(saln, name)
    qs, ds, pairs = edge_batch(letters, 0xE87E)
    classes = {saln.ends_free.pair_geometry(len(q)) for q in qs if q}
    assert classes == {(16, 10), (16, 16), (64, 8), (64, 16)}
    res, cig = compare(saln, qs, ds, pairs, sc, msc)
    assert sum(1 for k in range(len(pairs)) if len(cig[k]) > 3) >= 15   # alignments with gaps in them
    for k in range(len(pairs) - 4, len(pairs)):
        assert tuple(int(v) for v in res[k]) == (0, 0, 0, 0, 0, 0, 0, 0) and cig[k] == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_score_only_and_plan(saln, name):
    import torch
    from sequencealigning_amd import _lib
    sc, msc, letters = scoring(saln, name)
    qs, ds, pairs = edge_batch(letters, 0x5C0F)
    full, _ = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc)
    res, cig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, cigar=False)
    for k, (a, b) in enumerate(pairs):
        rec, _ = expect(qs[a], ds[b], msc, walk=False)
        assert tuple(int(v) for v in res[k]) == rec and cig[k] == []
    for f in ("score", "q_end", "db_end", "status"):
        assert (res[f] == full[f]).all()

    qb, qo = saln.pack_csr(qs)
    db, do = saln.pack_csr(ds)
    plan = saln.EndsFreePlan(qo, do, pairs, mode=EXTEND, scoring=sc)
    dq = torch.from_numpy(np.concatenate([qb, np.zeros(16, np.uint8)])).cuda()
    dd = torch.from_numpy(np.concatenate([db, np.zeros(16, np.uint8)])).cuda()
    out = [torch.full((plan.n_pairs * 8,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
    for o in out:
        plan.execute(dq, dd, o)
    torch.cuda.synchronize()
    got = [o.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE) for o in out]
    plan.close()
    assert (got[0] == got[1]).all()
    assert (got[0] == res).all()


# ------------------------------------------------------------------ 2. the borders
def _s(n=200):
    return rand_seq(random.Random(0x5EED), n, b"ACGT")


@pytest.mark.gpu
def test_leading_deletion(saln):
    """d = g junk bytes + s + tail, q = s: column 0 is a deletion run, and the
    path starts with gD (g = 63, 64, 65: around the lanes of a group)."""
    s, msc = _s(), model.scalar_scoring(*DEFAULT)
    tail = rand_seq(random.Random(7), 20, b"ACGT")
    gaps = (1, 63, 64, 65)
    qs, ds = [s], [b"N" * g + s + tail for g in gaps]     # N occurs in neither s nor the tail
    pairs = [(0, k) for k in range(len(gaps))]
    for g, d in zip(gaps, ds):
        a = model.align(s, d, EXTEND, msc)
        assert a.cigar == [(g, "D"), (200, "=")] and a.score == 1000 - 8 - 6 * g
    assert expect(s, ds[2], msc)[0][:6] == (608, 0, 0, 200, 0, 264)
    res, cig = compare(saln, qs, ds, pairs, DEFAULT, msc)
    assert [cig[k][0] for k in range(4)] == [(g, "D") for g in gaps]


@pytest.mark.gpu
def test_leading_insertion(saln):
    s, msc = _s(), model.scalar_scoring(*DEFAULT)
    q, d = b"N" * 10 + s[:100], s[:100]
    res, cig = compare(saln, [q], [d], [(0, 0)], DEFAULT, msc)
    assert cig[0] == [(10, "I"), (100, "=")] and int(res["score"][0]) == 432


@pytest.mark.gpu
def test_the_anchor_costs_more_than_it_earns(saln):
    s, msc = _s(), model.scalar_scoring(*DEFAULT)
    q, d = s[:70], b"N" * 64 + s[:70]
    res, cig = compare(saln, [q], [d], [(0, 0)], DEFAULT, msc)
    assert tuple(int(v) for v in res[0]) == (0, 0, 0, 0, 0, 0, 0, 0) and cig[0] == []
    loc, _ = saln.local_align(q, d, scoring=DEFAULT)
    assert int(loc["score"]) == 350


@pytest.mark.gpu
def test_pad_columns(saln):
    """q = s[:11] against d = s, 60 rows: five pad columns in lane 0 and every
    other lane past the query, below real cells that keep growing.  Then under
    a matrix that is positive everywhere: only the table's pad column keeps the
    pad cells below the real ones."""
    s = _s(60)
    msc = model.scalar_scoring(*DEFAULT)
    res, cig = compare(saln, [s[:11]], [s], [(0, 0)], DEFAULT, msc)
    assert tuple(int(v) for v in res[0])[:6] == (55, 0, 0, 11, 0, 11)
    table = [[3 + (a * 5 + b * 3) % 7 for b in range(4)] for a in range(4)]
    assert min(min(r) for r in table) > 0
    sm = saln.SubstitutionMatrix(b"ACGT", table, -1, -1)
    pmsc = model.matrix_scoring(b"ACGT", table, -1, -1)
    rng = random.Random(0x9AD)
    qs = [s[:11], rand_seq(rng, 9, b"ACGT"), rand_seq(rng, 161, b"ACGTN"), rand_seq(rng, 513, b"ACGT")]
    ds = [s, rand_seq(rng, 90, b"ACGTN"), rand_seq(rng, 200, b"ACGT"), rand_seq(rng, 65, b"ACGT")]
    res, cig = compare(saln, qs, ds, [(k, k) for k in range(4)], sm, pmsc)
    assert int(res["q_end"][0]) == 11 and int(res["db_end"][0]) >= 11
    sres, _ = saln.ends_free_align_batch(qs, ds, [(k, k) for k in range(4)], mode=EXTEND, scoring=sm, cigar=False)
    for f in ("score", "q_end", "db_end"):
        assert (sres[f] == res[f]).all()


# ------------------------------------------------------------------ 3. the scalar engine, direction
@pytest.mark.gpu
def test_match_mismatch_matrix_equals_the_scalar_engine(saln):
    table = [[5 if a == b else -4 for b in range(4)] for a in range(4)]
    sm = saln.SubstitutionMatrix(b"ACGT", table, -8, -6)
    rng = random.Random(0xEF08)
    qs = [rand_seq(rng, rng.randint(0, 60), b"ACGT") for _ in range(200)]
    ds = [anchored(rng, q, rng.randint(0, 60), b"ACGT") for q in qs]
    pairs = [(k, k) for k in range(200)]
    big = [rand_seq(rng, n, b"ACGT") for n in (150, 161, 300, 512, 700, 1024)]
    for a, q in enumerate(big):
        pairs.append((len(qs) + a, len(ds)))
        ds.append(anchored(rng, q, 150, b"ACGT"))
    qs += big
    for cigar in (True, False):
        want, wcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=DEFAULT, cigar=cigar)
        got, gcig = saln.ends_free_align_batch(qs, ds, pairs, mode=EXTEND, scoring=sm, cigar=cigar)
        assert (got == want).all()
        assert [gcig.words(k).tolist() for k in range(len(pairs))] == \
            [wcig.words(k).tolist() for k in range(len(pairs))]
    assert int((want["score"] != 0).sum()) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCORINGS)
def test_direction_left(saln, name):
    """direction="left": the model on the reversed inputs, mapped back; the
    matrix is not transposed."""
    sc, msc, letters = scoring(saln, name)
    rng = random.Random(0x1EF7)
    for n, m in ((40, 60), (300, 90), (11, 11), (5, 0)):
        q = rand_seq(rng, n, letters)
        d = anchored(rng, q[::-1], m, letters)[::-1]       # related at the right ends
        want = model.left_coords(model.align(q[::-1], d[::-1], EXTEND, msc), n, m)
        rec, cigar = saln.extend_align(q, d, scoring=sc, direction="left")
        assert tuple(int(v) for v in rec) == want.record() and cigar == want.cigar
        assert saln.alignment_score(q, d, (rec, cigar), sc) == want.score
        rrec, rcigar = saln.extend_align(q[::-1], d[::-1], scoring=sc)
        assert int(rrec["score"]) == want.score and rcigar == cigar[::-1]
    with pytest.raises(ValueError):
        saln.extend_align(b"A", b"A", direction="up")


# ------------------------------------------------------------------ 4. the longest db, the refusals
@pytest.mark.gpu
def test_the_longest_db_of_the_class_fills(saln):
    """65,000 rows, score only: column 0 runs down to o + 65,000 e."""
    sc, msc, letters = scoring(saln, "default")
    rng = random.Random(0x65008)
    qs = [rand_seq(rng, 9, letters), rand_seq(rng, 300, letters)]
    ds = [anchored(rng, qs[1], 400, letters) + rand_seq(rng, 64600, letters)]
    res, _ = saln.ends_free_align_batch(qs, ds, None, mode=EXTEND, scoring=sc, cigar=False)
    for k in range(2):
        score, q_end, db_end = model.linear_ends(qs[k], ds[0], EXTEND, msc)
        assert tuple(int(v) for v in res[k]) == (score, 0, -1, q_end, -1, db_end, 0, 0)
    assert int(res["score"][1]) > 500


@pytest.mark.gpu
def test_other_modes_are_still_refused(saln):
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    q, d = [b"ACGACG"], [b"ACGGACG"]
    res, cig = ef.ends_free_align_batch(q, d, mode=8)
    assert int(res["status"][0]) == 0 and int(res["score"][0]) > 0
    for mode in (0, 3, 5, -1):
        for call in (lambda: ef.ends_free_align_batch(q, d, mode=mode),
                     lambda: ef.ends_free_align_long_batch(q, d, mode=mode),
                     lambda: ef.ends_free_align_long_batch(q, d, mode=mode, replay=True),
                     lambda: ef.EndsFreePlan(np.array([0, 6], np.uint64), np.array([0, 7], np.uint64), mode=mode)):
            with pytest.raises(_lib.SalnError) as e:
                call()
            assert e.value.code == _lib.E_INVALID
            assert ("saln_nw_" if mode == 0 else "unknown mode %d" % mode) in _lib.last_error()
    plan = ef.EndsFreePlan(np.array([0, 6], np.uint64), np.array([0, 7], np.uint64), mode=8)
    plan.close()
