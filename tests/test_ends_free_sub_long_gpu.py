"""GPU: the chunked fill and the tiled replay of the ends-free engine under a
substitution matrix (the kSub instances of ends_free_long_kernels.hip and
ends_free_replay_kernels.hip through saln_ends_free_sub_long_align_batch and
saln_ends_free_sub_replay_align_batch).  Every comparison is exact against the
plain model (ends_free_model.py); the inputs' preconditions (each path
crosses a chunk edge and a tile edge) are asserted from the model first, and
without a device in test_the_paths_cross_chunk_and_tile_edges."""
import random

import pytest

import ends_free_model as model
import test_ends_free_sub_gpu as sg

LOCAL, SEMI, OVERLAP = model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP
MODES = [LOCAL, SEMI, OVERLAP]
CHUNK, TILE_ROWS = 1024, 64

# The 3-symbol matrix over its own letters, and a 24-symbol one shaped like a
# protein matrix (asymmetric; a symbol against itself 4 .. 11, against another
# -8 .. 2): related windows align, unrelated ones do not, so that a path can be
# made to lie over a chunk edge.
_rng = random.Random(0x24B2)
TABLE24P = [[_rng.randint(4, 11) if a == b else _rng.randint(-8, 2) for b in range(24)] for a in range(24)]
MATRICES = {
    "m3": (sg.ALPHABET3, sg.TABLE3, sg.GAPS3, sg.ALPHABET3),
    "p24": (sg.ALPHABET24, TABLE24P, (-10, -2), sg.ALPHABET24),
}


def model_scoring(name):
    alphabet, table, (o, e), letters = MATRICES[name]
    return model.matrix_scoring(alphabet, table, o, e), letters


def long_pairs(name):
    """1,025 x 70 and 2,049 x 130: a last chunk of one column, more rows than
    the 64 of a refill (and of a tile at tile_rows = 64), 130 more than the
    128-byte ring.  Each db is a window of its query over a chunk edge: the
    query's last 70 or 130 columns (the one-column chunk; both end in the same
    eight symbols that score well against themselves, so that an alignment
    keeps the last column), and 130 columns around column 1,024."""
    msc, letters = model_scoring(name)
    rng = random.Random(0x10C6)
    x, y = [bytes([c]) for c in letters if msc.S[c][c] >= 3][:2]
    tail = x + x + y + x + y + y + x + y
    q1, q2 = sg.rand_seq(rng, 1017, letters) + tail, sg.rand_seq(rng, 2041, letters) + tail
    qs = [q1, q2, q2]
    ds = [sg.mutated(rng, q1[1025 - 72:-8], 62, letters) + tail,
          sg.mutated(rng, q2[2049 - 134:-8], 122, letters) + tail,
          sg.mutated(rng, q2[960:1094], 130, letters)]
    assert [(len(q), len(d)) for q, d in zip(qs, ds)] == [(1025, 70), (2049, 130), (2049, 130)]
    return qs, ds


_expected = {}   # (name, mode) -> [(record, words, path)]: every model run happens once


def expected(name, mode):
    """The model's alignments of long_pairs, each asserted to cross a chunk
    edge (its path stands in two chunks) and a tile edge upwards (two row
    blocks of TILE_ROWS), with a step left over a chunk edge and a step up
    over a row-block edge."""
    if (name, mode) not in _expected:
        msc, _ = model_scoring(name)
        qs, ds = long_pairs(name)
        out = []
        for q, d in zip(qs, ds):
            path = []
            a = model.align(q, d, mode, msc, path=path)
            cells = [(i, j) for i, j in path if i >= 1 and j >= 1]
            chunks = [(j - 1) // CHUNK for _, j in cells]
            blocks = [(i - 1) // TILE_ROWS for i, _ in cells]
            assert len(set(chunks)) >= 2 and len(set(blocks)) >= 2, (len(q), len(d), mode)
            assert any(x > y for x, y in zip(chunks, chunks[1:])), "no step left over a chunk edge"
            assert any(x > y for x, y in zip(blocks, blocks[1:])), "no step up over a tile edge"
            out.append((a.record(), model.cigar_words(a.cigar)))
        _expected[(name, mode)] = out
    return _expected[(name, mode)]


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("mode", MODES)
def test_the_paths_cross_chunk_and_tile_edges(mode, name):
    assert len(expected(name, mode)) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("mode", MODES)
def test_chunked_fill_and_replay(saln, mode, name):
    from sequencealigning_amd import _lib
    want = expected(name, mode)
    sm, msc, _ = sg.scoring(saln, name, MATRICES)
    qs, ds = long_pairs(name)
    pairs = [(k, k) for k in range(3)]
    ef = saln.ends_free
    for q, d in zip(qs, ds):
        assert ef.pair_path_long(len(q), len(d))[0] == 1
    res, cig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sm)
    with _lib.options(**{"ends_free.tile_rows": TILE_ROWS}):
        rres, rcig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sm, replay=True)
    sres, scig = ef.ends_free_align_long_batch(qs, ds, pairs, mode=mode, scoring=sm, cigar=False)
    for k in range(3):
        rec, words = want[k]
        assert rcig.words(k).tolist() == cig.words(k).tolist(), k      # the replay's words are the long entry point's
        assert tuple(int(v) for v in rres[k]) == tuple(int(v) for v in res[k]), k
        assert tuple(int(v) for v in res[k]) == rec, k                 # and both are the model's
        assert cig.words(k).tolist() == words, k
        assert tuple(int(v) for v in sres[k]) == (rec[0], 0, -1, rec[3], -1, rec[5], 0, 0) and scig[k] == []
        assert saln.alignment_score(qs[k], ds[k], (res[k], cig[k]), sm) == rec[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_db_above_the_class_limit_score_only(saln, mode):
    """40 x 65,001: the chunked fill on the db-limit side, one chunk."""
    sm, msc, letters = sg.scoring(saln, "p24", MATRICES)
    rng = random.Random(0x65001 + mode)
    q = sg.rand_seq(rng, 40, letters)
    d = bytearray(sg.rand_seq(rng, 65001, letters))
    d[64950:64990] = sg.mutated(rng, q, 40, letters)
    d = bytes(d)
    assert saln.ends_free.pair_path_long(40, 65001) == (1, 1)
    res, cig = saln.ends_free.ends_free_align_long_batch([q], [d], mode=mode, scoring=sm, cigar=False)
    score, q_end, db_end = model.linear_ends(q, d, mode, msc)
    assert tuple(int(v) for v in res[0]) == (score, 0, -1, q_end, -1, db_end, 0, 0) and cig[0] == []
