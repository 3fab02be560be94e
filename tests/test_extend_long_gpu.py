"""GPU: extension mode (SALN_MODE_EXTEND) through the chunked fill with the
full trace and through the tiled replay at ends_free.tile_rows = 64
(ends_free_long_kernels.hip, ends_free_replay_kernels.hip).  Both equal the
plain model (ends_free_model.py), record for record and word for word, and each
other; the inputs' preconditions (a path over a chunk edge and a tile edge,
column 0 over tile edges, row 0 past a chunk edge) are asserted from the model
first, and without a device in test_the_paths_are_what_the_cases_need."""
import random

import pytest

import ends_free_model as model
import test_extend_gpu as eg

EXTEND = model.EXTEND
CHUNK, TILE_ROWS = 1024, 64
# Gaps cheap against a match, so that an alignment pinned at the origin reaches
# a column behind a chunk edge within 70 or 130 rows: through a long insertion.
CHEAP = (40, -36, -2, -1)
ROW0 = (5, -4, -2, -1)
# The same shape as a matrix: a symbol against itself 100 .. 120, against
# another -60 .. -20, asymmetric.
_rng = random.Random(0x24E9)
TABLE24X = [[_rng.randint(100, 120) if a == b else _rng.randint(-60, -20) for b in range(24)] for a in range(24)]
GAPS24X = (-2, -1)


def scoring(saln, name):
    """(the engine's scoring argument, the model's Scoring, the letters)."""
    if name == "x24":
        sm = saln.SubstitutionMatrix(eg.ALPHABET24, TABLE24X, *GAPS24X) if saln else None
        return sm, model.matrix_scoring(eg.ALPHABET24, TABLE24X, *GAPS24X), eg.ALPHABET24
    scheme = {"cheap": CHEAP, "row0": ROW0, "default": eg.DEFAULT}[name]
    return scheme, model.scalar_scoring(*scheme), b"ACGT"


def _mutate(rng, w, letters):
    """w with a few substitutions, its first and last eight bytes kept."""
    out = bytearray(w)
    for k in range(8, len(w) - 8):
        if rng.random() < 0.06:
            out[k] = rng.choice(letters)
    return bytes(out)


def crossing_pairs(letters):
    """1,025 x 70 and 2,049 x 130: a last chunk of one column, more rows than
    the 64 of a refill and of a tile, 130 more than the 128-byte ring.  The
    query is a + junk + b and the db a' + b': the path runs down a's diagonal,
    along one insertion over the junk (in the second pair over the chunk edge
    at column 1,024), and down b's diagonal into the one-column chunk."""
    rng = random.Random(0x10C8)
    junk = bytes([next(c for c in range(33, 127) if c not in letters)])
    out = []
    for n, m, la in ((1025, 70, 30), (2049, 130, 60)):
        a, b = eg.rand_seq(rng, la, letters), eg.rand_seq(rng, m - la, letters)
        q = a + junk * (n - m) + b
        d = _mutate(rng, a, letters) + _mutate(rng, b, letters)
        assert (len(q), len(d)) == (n, m)
        out.append((q, d))
    return out


def border_pairs():
    """Leading deletions of 64, 65 and 130 rows before a 1,100-column match
    (column 0 across the tile edges at rows 64 and 128, under the default
    scoring), and row 0 past a chunk edge: 1,030 junk columns before s."""
    rng = random.Random(0xB08D)
    s = eg.rand_seq(rng, 1100, b"ACGT")
    dele = [(s, b"N" * g + s) for g in (64, 65, 130)]
    t = eg.rand_seq(rng, 300, b"ACGT")
    return dele, (b"N" * 1030 + t, t)


_expected = {}   # every model run happens once


def expected(key):
    """[(record, words)] of the model for a group of pairs, each group's
    preconditions asserted."""
    if key in _expected:
        return _expected[key]
    out = []
    if key in ("cheap", "x24"):
        _, msc, letters = scoring(None, key)
        for q, d in crossing_pairs(letters):
            path = []
            a = model.align(q, d, EXTEND, msc, path=path)
            assert path[-1] == (0, 0) and a.score > 0
            cells = [(i, j) for i, j in path if i >= 1 and j >= 1]
            chunks = [(j - 1) // CHUNK for _, j in cells]
            blocks = [(i - 1) // TILE_ROWS for i, _ in cells]
            assert len(set(chunks)) >= 2 and len(set(blocks)) >= 2, (len(q), len(d))
            assert any(x > y for x, y in zip(chunks, chunks[1:])), "no step left over a chunk edge"
            assert any(x > y for x, y in zip(blocks, blocks[1:])), "no step up over a tile edge"
            assert (a.q_end, a.db_end) == (len(q), len(d))
            out.append((q, d, a.record(), model.cigar_words(a.cigar)))
    elif key == "deletions":
        msc = model.scalar_scoring(*eg.DEFAULT)
        for (q, d), g in zip(border_pairs()[0], (64, 65, 130)):
            a = model.align(q, d, EXTEND, msc)
            assert a.cigar == [(g, "D"), (1100, "=")] and a.score == 5500 - 8 - 6 * g
            out.append((q, d, a.record(), model.cigar_words(a.cigar)))
    else:
        msc = model.scalar_scoring(*ROW0)
        q, d = border_pairs()[1]
        a = model.align(q, d, EXTEND, msc)
        assert a.cigar == [(1030, "I"), (300, "=")] and a.record()[:6] == (468, 0, 0, 1330, 0, 300)
        out.append((q, d, a.record(), model.cigar_words(a.cigar)))
    _expected[key] = out
    return out


CASES = {"cheap": "cheap", "x24": "x24", "deletions": "default", "row0": "row0"}


@pytest.mark.parametrize("key", list(CASES))
def test_the_paths_are_what_the_cases_need(key):
    assert len(expected(key)) in (1, 2, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_chunked_fill_and_replay(saln, key):
    from sequencealigning_amd import _lib
    want = expected(key)
    sc, _, _ = scoring(saln, CASES[key])
    qs, ds = [w[0] for w in want], [w[1] for w in want]
    pairs = [(k, k) for k in range(len(want))]
    ef = saln.ends_free
    for q, d in zip(qs, ds):
        assert ef.pair_path_long(len(q), len(d))[0] == 1
    res, cig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=EXTEND, scoring=sc)
    with _lib.options(**{"ends_free.tile_rows": TILE_ROWS}):
        rres, rcig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, replay=True)
    sres, scig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=EXTEND, scoring=sc, cigar=False)
    for k, (q, d, rec, words) in enumerate(want):
        assert rcig.words(k).tolist() == cig.words(k).tolist(), k      # the replay's words are the long entry point's
        assert tuple(int(v) for v in rres[k]) == tuple(int(v) for v in res[k]), k
        assert tuple(int(v) for v in res[k]) == rec, k                 # and both are the model's
        assert cig.words(k).tolist() == words, k
        assert tuple(int(v) for v in sres[k]) == (rec[0], 0, -1, rec[3], -1, rec[5], 0, 0) and scig[k] == []
        assert saln.alignment_score(q, d, (res[k], cig[k]), sc) == rec[0]


@pytest.mark.gpu
def test_extend_align_long_both_directions(saln):
    """The one-pair form over the chunked path, with and without the replay,
    rightwards and leftwards."""
    from sequencealigning_amd import _lib
    q, d, rec, words = expected("row0")[0]
    for replay in (False, True):
        with _lib.options(**{"ends_free.tile_rows": TILE_ROWS}):
            r, c = saln.extend_align_long(q, d, scoring=ROW0, replay=replay)
            lr, lc = saln.extend_align_long(q[::-1], d[::-1], scoring=ROW0, replay=replay, direction="left")
        assert tuple(int(v) for v in r) == rec and c == [(1030, "I"), (300, "=")]
        assert tuple(int(v) for v in lr)[:6] == (468, 0, 0, 1330, 0, 300) and lc == c[::-1]


@pytest.mark.gpu
def test_db_above_the_class_limit_score_only(saln):
    """40 x 65,001: the chunked fill on the db-limit side, one chunk."""
    sc, msc, letters = eg.scoring(saln, "m24")
    rng = random.Random(0x65009)
    q = eg.rand_seq(rng, 40, letters)
    d = eg.anchored(rng, q, 60, letters) + eg.rand_seq(rng, 64941, letters)
    assert saln.ends_free.pair_path_long(40, 65001) == (1, 1)
    res, cig = saln.ends_free.ends_free_align_long_batch([q], [d], mode=EXTEND, scoring=sc, cigar=False)
    score, q_end, db_end = model.linear_ends(q, d, EXTEND, msc)
    assert tuple(int(v) for v in res[0]) == (score, 0, -1, q_end, -1, db_end, 0, 0) and cig[0] == []
    assert score > 0
