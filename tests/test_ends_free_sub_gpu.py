"""GPU: the ends-free engine under a substitution matrix (the kSub instances
of ends_free_kernels.hip through saln_ends_free_sub_*), local, semi-global and
overlap.  Every comparison is exact against the plain model
(ends_free_model.py): the whole result record and the CIGAR, word for
word; and alignment_score of every returned alignment is its score."""
import ctypes
import random

import numpy as np
import pytest

import ends_free_model as model

LOCAL, SEMI, OVERLAP = model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP
MODES = [LOCAL, SEMI, OVERLAP]

# The 3-symbol matrix of test_ends_free_sub_model.py: asymmetric, a zero entry,
# a negative diagonal entry, a positive off-diagonal entry.
ALPHABET3 = b"ACG"
TABLE3 = [[4, -3, 2], [-2, 3, 0], [-4, -5, -1]]
GAPS3 = (-3, -1)
# 24 symbols (a protein alphabet's size), random asymmetric entries in -8 .. 11.
ALPHABET24 = b"ARNDCQEGHILKMFPSTWYVBZXU"
_rng24 = random.Random(0x24B1)
TABLE24 = [[_rng24.randint(-8, 11) for _ in range(24)] for _ in range(24)]
GAPS24 = (-10, -2)
assert any(TABLE24[a][b] != TABLE24[b][a] for a in range(24) for b in range(24))
assert min(min(r) for r in TABLE24) == -8 and max(max(r) for r in TABLE24) == 11

MATRICES = {
    "m3": (ALPHABET3, TABLE3, GAPS3, b"ACGT"),          # T: outside the alphabet
    "m24": (ALPHABET24, TABLE24, GAPS24, ALPHABET24 + b"O"),
}


def scoring(saln, name, matrices=MATRICES, **kw):
    """(SubstitutionMatrix, the model's Scoring, the bytes sequences draw from)."""
    alphabet, table, (o, e), letters = matrices[name]
    return (saln.SubstitutionMatrix(alphabet, table, o, e, **kw),
            model.matrix_scoring(alphabet, table, o, e, **kw), letters)


def rand_seq(rng, n, letters):
    return bytes(rng.choice(letters) for _ in range(n))


def mutated(rng, src, length, letters):
    """`length` bytes: a window of src with 8 % substitutions and a few indels."""
    if not src:
        return rand_seq(rng, length, letters)
    i = rng.randrange(max(1, len(src) - length + 1))
    out = bytearray()
    while len(out) < length:
        u = rng.random()
        if u < 0.08:
            out.append(rng.choice(letters))
            i += 1
        elif u < 0.095:
            i += rng.randint(1, 3)                           # deletion
        elif u < 0.11:
            out += rand_seq(rng, rng.randint(1, 3), letters)  # insertion
        else:
            out.append(src[i % len(src)])
            i += 1
    return bytes(out[:length])


def expect(q, d, mode, msc, walk=True):
    a = model.align(q, d, mode, msc, walk=walk)
    return a.record(), model.cigar_words(a.cigar)


def compare(saln, qs, ds, pairs, mode, sm, msc, batch=None, **kw):
    """Runs one batch and compares every pair with the model and with
    alignment_score."""
    batch = batch or saln.ends_free_align_batch
    res, cig = batch(qs, ds, pairs, mode=mode, scoring=sm, **kw)
    plist = pairs if pairs is not None else [(a, b) for b in range(len(ds)) for a in range(len(qs))]
    assert len(res) == len(cig) == len(plist)
    for k, (a, b) in enumerate(plist):
        rec, words = expect(qs[a], ds[b], mode, msc)
        assert tuple(int(v) for v in res[k]) == rec, (k, len(qs[a]), len(ds[b]), qs[a][:40], ds[b][:40])
        assert cig.words(k).tolist() == words, (k, qs[a][:40], ds[b][:40])
        assert saln.alignment_score(qs[a], ds[b], (res[k], cig[k]), sm) == int(res["score"][k]), k
    return res, cig


# ------------------------------------------------------------------ 1. class edges
EDGE_QUERIES = (1, 9, 10, 11, 160, 161, 256, 257, 512, 513, 1024)
EDGE_DBS = (1, 2, 15, 16, 17, 63, 64, 65, 90)


def edge_batch(letters, seed):
    """Every class, pad columns in each (9, 11, 161, 257, 513 are no multiple
    of their class's columns per lane) and full last lanes (10, 160, 256, 512,
    1024); dbs of 1 to 90 rows, related to the query and not."""
    rng = random.Random(seed)
    qs = [rand_seq(rng, n, letters) for n in EDGE_QUERIES]
    ds, pairs = [], []
    for a, q in enumerate(qs):
        for m in EDGE_DBS:
            pairs.append((a, len(ds)))
            ds.append(mutated(rng, q, m, letters) if (a + m) % 3 else rand_seq(rng, m, letters))
    # the last columns of the query: the lane that owns column lq decides
    for a, q in enumerate(qs):
        pairs.append((a, len(ds)))
        ds.append(mutated(rng, q[-40:], min(len(q), 40), letters))
    return qs, ds, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("mode", MODES)
def test_class_edges(saln, mode, name):
    sm, msc, letters = scoring(saln, name)
    qs, ds, pairs = edge_batch(letters, 0xED6E)
    classes = {saln.ends_free.pair_geometry(len(q)) for q in qs}
    assert classes == {(16, 10), (16, 16), (64, 8), (64, 16)}
    res, cig = compare(saln, qs, ds, pairs, mode, sm, msc)
    assert sum(1 for k in range(len(pairs)) if len(cig[k]) > 3) >= 20   # alignments with gaps in them


# ------------------------------------------------------------------ 2. the scalar engine
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_match_mismatch_matrix_equals_the_scalar_engine(saln, mode):
    """The differential test against the kernels without kSub: a matrix that
    encodes (5, -4, -8, -6) over ACGT gives their records and words."""
    scheme = (5, -4, -8, -6)
    table = [[5 if a == b else -4 for b in range(4)] for a in range(4)]
    sm = saln.SubstitutionMatrix(b"ACGT", table, -8, -6)
    rng = random.Random(0xEF00 + 4)
    qs = [rand_seq(rng, rng.randint(0, 40), b"ACGT") for _ in range(300)]
    ds = [rand_seq(rng, rng.randint(0, 40), b"ACGT") for _ in range(300)]
    pairs = [(k, k) for k in range(300)]
    # and every class: the mixed batch of test_ends_free_gpu.py's shape
    big = [rand_seq(rng, n, b"ACGT") for n in (0, 7, 150, 161, 200, 300, 512, 700, 1024)]
    for b, (src, m) in enumerate(((2, 150), (6, 400), (0, 0), (8, 90))):
        d = mutated(rng, big[src], m, b"ACGT")
        for a in range(len(big)):
            pairs.append((len(qs) + a, len(ds)))
        ds.append(d)
    qs += big
    for cigar in (True, False):
        want, wcig = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=scheme, cigar=cigar)
        got, gcig = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=sm, cigar=cigar)
        assert (got == want).all()
        assert [gcig.words(k).tolist() for k in range(len(pairs))] == \
            [wcig.words(k).tolist() for k in range(len(pairs))]
    assert int((want["score"] != 0).sum()) > 250


# ------------------------------------------------------------------ 3. symbols and bytes
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_byte_outside_the_alphabet_scores_unknown(saln, mode):
    for unknown in (None, -7, 6):
        kw = {} if unknown is None else {"unknown": unknown}
        sm, msc, _ = scoring(saln, "m3", **kw)
        u = -5 if unknown is None else unknown
        rng = random.Random(0x0171 + mode)
        qs = [b"ATA", b"TTTT", b"\x00\xffA", b"AtA"] + [rand_seq(rng, rng.randint(1, 60), b"ACGTNacg\x00\xff")
                                                        for _ in range(60)]
        ds = [b"ATA", b"TTTT", b"\xff\x00A", b"ATA"] + [mutated(rng, q, rng.randint(1, 70), b"ACGTNacg\x00\xff")
                                                        for q in qs[4:]]
        res, cig = compare(saln, qs, ds, [(k, k) for k in range(len(qs))], mode, sm, msc)
        if mode == SEMI:
            assert (int(res["score"][0]), cig[0]) == (4 + u + 4, [(3, "=")])
            assert (int(res["score"][3]), cig[3]) == (4 + u + 4, [(1, "="), (1, "X"), (1, "=")])   # t is not T
        if mode == LOCAL and u > 0:
            assert (int(res["score"][1]), cig[1]) == (4 * u, [(4, "=")])
            assert (int(res["score"][2]), cig[2]) == (2 * u + 4, [(2, "X"), (1, "=")])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_positive_score_without_a_shared_byte(saln, mode):
    """db A against query G scores 2: every column is 'X' and the score is
    positive; the transposed pair (db G against query A: -4) scores nothing."""
    sm, msc, _ = scoring(saln, "m3")
    qs = [b"GGGG", b"AAAA", b"G" * 300, b"G" * 1024]
    ds = [b"AAAA", b"GGGG", b"A" * 70, b"A" * 90]
    res, cig = compare(saln, qs, ds, [(k, k) for k in range(4)], mode, sm, msc)
    assert (int(res["score"][0]), cig[0]) == (8, [(4, "X")])
    if mode != SEMI:     # the db inside the query: semi-global pays for the rest of the query
        assert cig[2] == [(70, "X")] and int(res["score"][2]) == 140
        assert cig[3] == [(90, "X")] and int(res["score"][3]) == 180
    if mode == SEMI:
        assert int(res["score"][1]) < 0
    else:
        assert tuple(int(v) for v in res[1]) == (0, 0, 0, 0, 0, 0, 0, 0) and cig[1] == []


def test_case_insensitive_on_the_model_side():
    assert model.matrix_scoring(b"A", [[2]], -1, -1, case_insensitive=True).S[ord("a")][ord("A")] == 2


@pytest.mark.gpu
def test_case_insensitive(saln):
    sm = saln.SubstitutionMatrix(ALPHABET3, TABLE3, *GAPS3, case_insensitive=True)
    msc = model.matrix_scoring(ALPHABET3, TABLE3, *GAPS3, case_insensitive=True)
    res, cig = compare(saln, [b"acgACG"], [b"ACGacg"], [(0, 0)], LOCAL, sm, msc)
    assert (int(res["score"][0]), cig[0]) == (4 + 3 - 1 + 4 + 3, [(5, "X")])   # the last G on g scores -1


# ------------------------------------------------------------------ 4. score only, the plan
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("mode", MODES)
def test_score_only_and_plan(saln, mode, name):
    import torch
    from sequencealigning_amd import _lib
    sm, msc, letters = scoring(saln, name)
    qs, ds, pairs = edge_batch(letters, 0x5C0E)
    full, _ = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=sm)
    res, cig = saln.ends_free_align_batch(qs, ds, pairs, mode=mode, scoring=sm, cigar=False)
    for k, (a, b) in enumerate(pairs):
        rec, _ = expect(qs[a], ds[b], mode, msc, walk=False)
        assert tuple(int(v) for v in res[k]) == rec and cig[k] == []
    for f in ("score", "q_end", "db_end", "status"):
        assert (res[f] == full[f]).all()

    qb, qo = saln.pack_csr(qs)
    db, do = saln.pack_csr(ds)
    plan = saln.EndsFreePlan(qo, do, pairs, mode=mode, scoring=sm)
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


@pytest.mark.gpu
def test_the_longest_db_of_the_class_fills(saln):
    """65,000 rows, the classes' limit: the staged row and the matrix's block
    together are the most LDS a workgroup of these fills asks for, in a group
    of 16 lanes and in one of 64."""
    sm, msc, letters = scoring(saln, "m24")
    rng = random.Random(0x65000)
    qs = [rand_seq(rng, 9, letters), rand_seq(rng, 170, letters)]
    d = bytearray(rand_seq(rng, 65000, letters))
    d[64000:64009] = qs[0]
    d[64500:64670] = qs[1]
    res, _ = saln.ends_free_align_batch(qs, [bytes(d)], None, mode=LOCAL, scoring=sm, cigar=False)
    for k in range(2):
        score, q_end, db_end = model.linear_ends(qs[k], bytes(d), LOCAL, msc)
        assert (int(res["score"][k]), int(res["q_end"][k]), int(res["db_end"][k])) == (score, q_end, db_end)
        assert score > 0


# ------------------------------------------------------------------ 5. refusals
def _refused(fn):
    from sequencealigning_amd import _lib
    with pytest.raises(_lib.SalnError) as e:
        fn()
    assert e.value.code == _lib.E_INVALID
    assert _lib.last_error() != ""
    return _lib.last_error()


@pytest.mark.gpu
def test_refusals(saln):
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    SM = saln.SubstitutionMatrix
    q, d = [b"ACGACG"], [b"ACGGACG"]
    ok = SM(ALPHABET3, TABLE3, *GAPS3)
    assert int(ef.ends_free_align_batch(q, d, mode=LOCAL, scoring=ok)[0]["status"][0]) == 0
    # an invalid matrix, through every entry point
    for bad in (SM(ALPHABET3, TABLE3, 1, -1), SM(ALPHABET3, TABLE3, -3, 0),
                SM(ALPHABET3, [[0, -1, -1]] * 3, -3, -1)):
        for mode in MODES:
            _refused(lambda: ef.ends_free_align_batch(q, d, mode=mode, scoring=bad))
        _refused(lambda: ef.ends_free_align_long_batch(q, d, mode=LOCAL, scoring=bad))
        _refused(lambda: ef.ends_free_align_long_batch(q, d, mode=LOCAL, scoring=bad, replay=True))
        _refused(lambda: ef.EndsFreePlan(np.array([0, 6], np.uint64), np.array([0, 7], np.uint64),
                                         mode=SEMI, scoring=bad))
    assert "saln_nw_" in _refused(lambda: ef.ends_free_align_batch(q, d, mode=saln.Mode.Global, scoring=ok))
    # the classes' limits are the scalar entry point's
    assert "1024" in _refused(lambda: ef.ends_free_align_batch([b"A" * 1025], d, mode=LOCAL, scoring=ok))
    # a NULL matrix: there is no default
    L = _lib.lib()
    qb, qo = saln.pack_csr(q)
    db, do = saln.pack_csr(d)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for entry in ("saln_ends_free_sub_align_batch", "saln_ends_free_sub_long_align_batch",
                  "saln_ends_free_sub_replay_align_batch"):
        h = ctypes.c_void_p()
        rc = getattr(L, entry)(_lib.context(0), vp(qb), vp(qo), 1, vp(db), vp(do), 1, None, None, 1, LOCAL,
                               None, 0, 1, ctypes.byref(h))
        assert rc == _lib.E_INVALID and not h.value and "NULL" in _lib.last_error(), entry
    h = ctypes.c_void_p()
    rc = L.saln_ends_free_sub_plan_create(_lib.context(0), vp(qo), 1, vp(do), 1, None, None, 1, LOCAL, None,
                                          ctypes.byref(h))
    assert rc == _lib.E_INVALID and not h.value
    # the range guard: (n + m + 2) * max|parameter| >= 2^30, the largest
    # |parameter| here a gap cost, then an entry
    wide = SM(ALPHABET3, TABLE3, -100000, -1)
    assert wide.check() == 100000 and 10738 * 100000 >= 1 << 30 > 10737 * 100000
    qa = [rand_seq(random.Random(1), 1024, b"ACG")]
    msg = _refused(lambda: ef.ends_free_align_batch(qa, [b"A" * 9712], mode=LOCAL, scoring=wide, cigar=False))
    assert "2^30" in msg
    res, _ = ef.ends_free_align_batch(qa, [qa[0] * 9 + b"A" * 495], mode=LOCAL, scoring=wide, cigar=False)
    msc = model.matrix_scoring(ALPHABET3, TABLE3, -100000, -1)
    assert int(res["score"][0]) == model.linear_ends(qa[0], qa[0] * 9 + b"A" * 495, LOCAL, msc)[0] > 1024
    entry = SM(ALPHABET3, [[127, -3, 2], [-2, 3, 0], [-4, -5, -128]], -3, -1)
    assert entry.check() == 128 and (1 << 23) * 128 == 1 << 30
    long_q = [bytes((1 << 23) - 2 - 7)]
    assert "2^30" in _refused(lambda: ef.ends_free_align_long_batch(long_q, d, mode=LOCAL, scoring=entry,
                                                                    cigar=False))
