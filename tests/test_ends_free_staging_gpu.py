"""GPU: the staging geometry of the class fills (launch_ef_fill in
ends_free_kernels.hip).  A launch packs 256 / lanes lane groups, one pair each,
into a workgroup and lowers that count until the groups' staged db rows,
groups * (ld_max + 2 * lanes) bytes, fit 64 KB (64 KB less the matrix's block
of 1,408 bytes under a substitution matrix).  saln_ends_free_fill_geometry,
which the launch asks, says what a launch gets; the launches here hit every
count between the full workgroup and one group:

    16 lanes   16, 15, 13, 2, 1 groups (workgroups of 256, 240, 208, 32, 16
               lanes: in a 240- or 208-lane workgroup the last wave is partly
               empty while the 16-lane ballot slice and row_shr are in use)
    64 lanes   4, 3, 2, 1 groups (256, 192, 128, 64 lanes)

each with and without a matrix, whose smaller budget moves every boundary.
ld_max is the largest db length that still gets the count, from the formula,
not from a table.

A launch holds 2 * groups + 1 pair entries (two full workgroups and a partly
filled one) over three or four distinct pairs: A and B with dbs of ld_max rows,
alternating, then C and D with dbs at the low end of ld_max's power-of-two
bucket (a batch is cut into launches by bucket), alternating: neighbouring
groups hold different pairs, and rows of different lengths share the stride of
ld_max.  Local's best cell lies in the db's last rows, so the score reads the
end of every staged row.  Every comparison is exact against the plain models;
X-drop launches end their pairs' homology at different rows, so the groups of
a wave leave the row loop at different steps, each within steps_bound."""
import functools
import random

import pytest

import ends_free_model as model
import xdrop_model
from test_extend_gpu import ALPHABET24, DEFAULT, GAPS24, TABLE24, anchored, rand_seq

LOCAL, EXTEND = model.LOCAL, model.EXTEND
LDS, SUB_BYTES = 64 << 10, 256 + 32 * 36
COUNTS = {16: (16, 15, 13, 2, 1), 64: (4, 3, 2, 1)}
CASES = [(lanes, g) for lanes in (16, 64) for g in COUNTS[lanes]]
XDROP = 40


def top_ld(lanes, groups, matrix):
    """The longest db of a launch that gets `groups` groups: the largest ld with
    groups * (ld + 2 lanes) within the budget; for one group, one row more than
    two groups take."""
    budget = LDS - (SUB_BYTES if matrix else 0)
    return budget // groups - 2 * lanes if groups > 1 else budget // 2 - 2 * lanes + 1


def scoring(saln, name):
    if name == "m24":
        return (saln.SubstitutionMatrix(ALPHABET24, TABLE24, *GAPS24),
                model.matrix_scoring(ALPHABET24, TABLE24, *GAPS24), ALPHABET24)
    return DEFAULT, model.scalar_scoring(*DEFAULT), b"ACGT"


def query_lengths(lanes, groups):
    """Two queries of one class: 16 x 10 or 16 x 16 by turns; 64 x 8 with words,
    64 x 16 (score only, the model with rolling rows) for the longest dbs."""
    if lanes == 16:
        return (150, 160) if groups in (16, 13, 1) else (200, 256)
    return (257, 300) if groups >= 3 else (1024, 600)


def rand_bytes(rng, n, letters):
    return bytes(rng.choices(letters, k=n))


def plain_db(rng, q, length, letters):
    """A mutated copy of q's prefix first (extension's alignment), random rows,
    and q itself in the last rows (local's best cell is in row `length`)."""
    head = anchored(rng, q, min(len(q), length // 4), letters)
    return head + rand_bytes(rng, length - len(head) - len(q), letters) + q


def xdrop_db(rng, q, length, hom, name, letters):
    """q's first `hom` bytes, then rows no extension survives (random bases; under
    the matrix, whose random entries average above 0, a byte outside the
    alphabet, which scores the smallest entry)."""
    junk = b"O" * (length - hom) if name == "m24" else rand_bytes(rng, length - hom, letters)
    return q[:hom] + junk


@functools.lru_cache(maxsize=None)
def launch(lanes, groups, name, xdrop):
    """(qs, ds, pairs, ld_max, distinct pairs) of one launch."""
    matrix = name == "m24"
    letters = ALPHABET24 if matrix else b"ACGT"
    ld_max = top_ld(lanes, groups, matrix)
    low = 1 << (ld_max.bit_length() - 1)
    rng = random.Random(0x57A6 + 1000 * lanes + 10 * groups + matrix + 2 * xdrop)
    na, nb = query_lengths(lanes, groups)
    lengths = [(na, ld_max), (nb, ld_max), (nb, low)] + ([(na, low)] if groups >= 3 else [])
    homs = (30, min(na, nb) - 10, 80, 5)
    qs, ds = [], []
    for k, (n, length) in enumerate(lengths):
        q = rand_seq(rng, n, letters)
        qs.append(q)
        ds.append(xdrop_db(rng, q, length, homs[k], name, letters) if xdrop else plain_db(rng, q, length, letters))
    # A, B alternating, then C (and D): the fills order a launch by falling db
    # length and keep the given order within one length
    n_low = groups if groups >= 3 else 1
    order = [k % 2 for k in range(2 * groups + 1 - n_low)] + [2 + k % (len(lengths) - 2) for k in range(n_low)]
    return qs, ds, [(k, k) for k in order], ld_max, len(lengths)


_memo = {}


def expect(q, d, fill, name, msc, walk):
    """The model's (Alignment, L), once per pair: with words from the full
    matrices, score only (the 64 x 16 launches) with rolling rows."""
    key = (q, d, fill, name, walk)
    if key not in _memo:
        if fill == "xdrop":
            a, _, L = xdrop_model.align(q, d, XDROP, msc, walk=walk)
        elif walk:
            a, L = model.align(q, d, LOCAL if fill == "local" else EXTEND, msc), None
        else:
            score, q_end, db_end = model.linear_ends(q, d, LOCAL if fill == "local" else EXTEND, msc)
            a, L = model.Alignment(score, -1, q_end, -1, db_end), None
        _memo[key] = (a, L)
    return _memo[key]


# ------------------------------------------------------------------ the geometry (host only)
def test_the_boundaries_follow_the_formula(saln):
    ef = saln.ends_free
    flips = {16: [], 64: []}
    for lanes, n in ((16, 100), (16, 200), (64, 400), (64, 1000)):
        assert ef.pair_geometry(n)[0] == lanes
        for matrix in (False, True):
            budget = LDS - (SUB_BYTES if matrix else 0)
            for g in range(256 // lanes, 1, -1):
                ld = budget // g - 2 * lanes
                assert ef.fill_geometry(n, ld, matrix) == (g, g * (ld + 2 * lanes)), (lanes, g, matrix)
                assert ef.fill_geometry(n, ld + 1, matrix)[0] == g - 1, (lanes, g, matrix)
                if not matrix and n in (100, 400):
                    flips[lanes].append((g, ld))
            for ld in (0, 1, 400):
                assert ef.fill_geometry(n, ld, matrix)[0] == 256 // lanes
            assert ef.fill_geometry(n, 65000, matrix) == (1, 65000 + 2 * lanes)
    assert {g: ld for g, ld in flips[16]}[16] == 4064 and dict(flips[16])[15] == 4337 and dict(flips[16])[2] == 32736
    assert dict(flips[64]) == {4: 16256, 3: 21717, 2: 32640}
    assert ef.fill_geometry(100, 4000) == (16, 16 * 4032) and ef.fill_geometry(100, 4000, True)[0] == 15


def test_every_count_is_hit_with_and_without_a_matrix(saln):
    ef = saln.ends_free
    for name in ("default", "m24"):
        hit = {16: set(), 64: set()}
        for lanes, groups in CASES:
            for xdrop in (False, True):
                qs, ds, pairs, ld_max, distinct = launch(lanes, groups, name, xdrop)
                assert {ef.pair_geometry(len(q)) for q in qs} in ({(16, 10)}, {(16, 16)}, {(64, 8)}, {(64, 16)})
                assert max(len(d) for d in ds) == ld_max and len(pairs) == 2 * groups + 1
                assert {len(d).bit_length() for d in ds} == {ld_max.bit_length()}       # one launch
                assert min(len(d) for d in ds) == 1 << (ld_max.bit_length() - 1)        # the bucket's low end
                got, lds = ef.fill_geometry(len(qs[0]), ld_max, name == "m24")
                assert got == groups and lds <= LDS - (SUB_BYTES if name == "m24" else 0)
                assert len({k for k, _ in pairs}) == distinct
            hit[lanes].add(got)
        assert hit == {16: {16, 15, 13, 2, 1}, 64: {4, 3, 2, 1}}
        assert {g * 16 for g in hit[16]} >= {240, 208} and {g * 64 for g in hit[64]} >= {192, 128}


# ------------------------------------------------------------------ the launches
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("default", "m24"))
@pytest.mark.parametrize("lanes, groups", CASES)
@pytest.mark.parametrize("fill", ("local", "extend", "xdrop"))
def test_launch(saln, fill, lanes, groups, name):
    sc, msc, _ = scoring(saln, name)
    xdrop = fill == "xdrop"
    qs, ds, pairs, ld_max, _ = launch(lanes, groups, name, xdrop)
    assert saln.ends_free.fill_geometry(len(qs[0]), ld_max, name == "m24")[0] == groups
    words = max(len(q) for q in qs) <= 512            # 64 x 16: score only
    kw = dict(mode=LOCAL if fill == "local" else EXTEND, scoring=sc, **({"xdrop": XDROP} if xdrop else {}))
    want = [expect(qs[k], ds[k], fill, name, msc, words) for k, _ in pairs]
    sres, scig = saln.ends_free_align_batch(qs, ds, pairs, cigar=False, **kw)
    for e, (k, _) in enumerate(pairs):
        a = want[e][0]
        ends = (a.score, 0, -1, a.q_end, -1, a.db_end, 0)
        assert tuple(int(v) for v in sres[e])[:7] == ends and scig[e] == [], (e, k, sres[e], ends)
    if words:
        res, cig = saln.ends_free_align_batch(qs, ds, pairs, **kw)
        for e, (k, _) in enumerate(pairs):
            a = want[e][0]
            assert tuple(int(v) for v in res[e])[:7] == a.record()[:7], (e, k, res[e], a.record())
            assert cig.words(e).tolist() == model.cigar_words(a.cigar), (e, k)
            assert saln.alignment_score(qs[k], ds[k], (res[e], cig[e]), sc) == a.score, (e, k)
        assert (res["reserved"] == sres["reserved"]).all()
    if fill == "local" and name == "default":
        # q itself ends the db: the best cell is in the last staged row of every stride (under the
        # matrix, whose random entries average above 0, the best cell is wherever the model says)
        assert all(int(sres["db_end"][e]) == len(ds[k]) and int(sres["q_end"][e]) == len(qs[k])
                   for e, (k, _) in enumerate(pairs))
    if fill == "extend":
        assert (sres["score"] > 0).all() and (sres["reserved"] == 0).all()
    if xdrop:
        steps = [int(v) for v in sres["reserved"]]
        for e, (k, _) in enumerate(pairs):
            L = want[e][1]
            most = xdrop_model.steps_bound(len(ds[k]), L, lanes)
            assert max(L, 1) <= steps[e] <= most, (e, k, steps[e], L, most)
        # A and B alternate in the first wave: its groups (16 lanes) or the
        # workgroup's waves (64) leave the row loop at different steps
        assert steps[0] != steps[1] and want[0][1] != want[1][1]
        assert max(steps) < ld_max // 8
