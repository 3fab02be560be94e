"""CPU: the oracle's scoring-scheme parameter (oracle/refcpu.c ref_nw_fill_s,
reflinear.c, refcheck.c) against a plain three-matrix fill written here from
the recurrences, in Python integers:

    M[x][y] = max(M, I, D)[x-1][y-1] + (match | mismatch)
    I[x][y] = max(M[x][y-1] + go, I[x][y-1]) + ge          (from the left)
    D[x][y] = max(M[x-1][y] + go, D[x-1][y]) + ge          (from above)
    M[0][0] = 0, every other boundary M/I/D = -32768 except
    D[0][y>=1] = (y+1) ge + go and I[x>=1][0] = go + (x+1) ge,

x over the db, y over the query.  Parent bits record every argument that
ties the maximum.  The default scheme's outputs stay the committed goldens."""
import json
import os

import numpy as np
import pytest

from nw_check import SCHEMES, SENTINEL_SCHEME, path_score, rand_seq

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SENT = -32768
OPS = {7: "=", 8: "X", 1: "I", 2: "D"}


def py_fill(q: bytes, d: bytes, scheme):
    """(M, I, D, parents, score, end_states): parents[x][y] holds the seven
    parent bits of the cell, bit0-2 M's parents {M, I, D}(x-1, y-1), bit3-4
    I's parents {I, M}(x, y-1), bit5-6 D's parents {D, M}(x-1, y)."""
    mat, mis, go, ge = scheme
    W, H = len(q) + 1, len(d) + 1
    M = [[SENT] * W for _ in range(H)]
    I = [[SENT] * W for _ in range(H)]
    D = [[SENT] * W for _ in range(H)]
    P = [[0] * W for _ in range(H)]
    M[0][0] = 0
    for y in range(1, W):
        D[0][y] = (y + 1) * ge + go
        P[0][y] = 32
    for x in range(1, H):
        I[x][0] = go + (x + 1) * ge
        P[x][0] = 8
    for x in range(1, H):
        for y in range(1, W):
            s = mat if q[y - 1] == d[x - 1] else mis
            dg = (M[x - 1][y - 1], I[x - 1][y - 1], D[x - 1][y - 1])
            m = max(dg) + s
            b = sum(1 << k for k in range(3) if dg[k] + s == m)
            lf = (I[x][y - 1] + ge, M[x][y - 1] + go + ge)
            iv = max(lf)
            b |= sum(8 << k for k in range(2) if lf[k] == iv)
            up = (D[x - 1][y] + ge, M[x - 1][y] + go + ge)
            dv = max(up)
            b |= sum(32 << k for k in range(2) if up[k] == dv)
            M[x][y], I[x][y], D[x][y], P[x][y] = m, iv, dv, b
    end = (M[-1][-1], I[-1][-1], D[-1][-1])
    score = max(end)
    return M, I, D, P, score, sum(1 << k for k in range(3) if end[k] == score)


def py_dense(M, I, D, P):
    """The dense cell code: bits0-2 the states that hold max(M, I, D) of the
    cell, bits3-4 I's parents, bits5-6 D's parents."""
    out = np.zeros((len(M), len(M[0])), np.uint8)
    for x in range(len(M)):
        for y in range(len(M[0])):
            v = (M[x][y], I[x][y], D[x][y])
            out[x, y] = sum(1 << k for k in range(3) if v[k] == max(v)) | (P[x][y] & 0x78)
    return out


def _check_against_py(oracle, q, d, s):
    o = oracle.nw(q, d, literal_dfs=False, scoring=s)
    M, I, D, P, score, es = py_fill(q, d, s)
    ctx = (s, q, d)
    assert o.M.tolist() == M, ctx
    assert o.I.tolist() == I, ctx
    assert o.D.tolist() == D, ctx
    assert (o.dense_mask == py_dense(M, I, D, P)).all(), ctx
    assert (o.score, o.end_states) == (score, es), ctx
    if o.first_ops is not None:
        sc, ok = path_score(q, d, [(1, c) for c in o.first_ops], s)
        assert ok and sc == o.score, ctx
    return o


def test_fill_matches_python_recurrences(oracle):
    rng = np.random.default_rng(101)
    schemes = list(SCHEMES)
    alphabets = [b"ACGT", b"ACGTN", b"AC"]
    printed = 0
    for k in range(10 * len(schemes)):
        s = schemes[k % len(schemes)]
        a = alphabets[(k // len(schemes)) % 3]
        q = rand_seq(rng, int(rng.integers(0, 25)), a)
        d = rand_seq(rng, int(rng.integers(0, 25)), a)
        printed += _check_against_py(oracle, q, d, s).first_ops is not None
    assert printed > 100
    # both sides at their extremes, and the empty sides, under every scheme
    for s in schemes:
        for q, d in [(b"", b""), (b"ACG", b""), (b"", b"ACG"), (b"A" * 24, b"A" * 24),
                     (b"AC" * 12, b"GT" * 12)]:
            _check_against_py(oracle, q, d, s)


def test_fill_matches_python_past_the_sentinel(oracle):
    """(5,-4,-8,-600): boundary values fall below -32768 at 54 columns, so the
    sentinel ties and wins inside the table and dead-end parent sets appear."""
    rng = np.random.default_rng(102)
    dead = 0
    for k in range(6):
        q = rand_seq(rng, int(rng.integers(50, 71)), b"ACGT" if k % 2 else b"AC")
        d = rand_seq(rng, int(rng.integers(50, 71)), b"ACGT" if k % 2 else b"AC")
        o = _check_against_py(oracle, q, d, SENTINEL_SCHEME)
        dead += (o.M[1:, 1:] < SENT // 2).any()
    assert dead


@pytest.mark.parametrize("scoring", [None, (5, -4, -8, -6)])
def test_default_scheme_reproduces_goldens(oracle, scoring):
    with open(os.path.join(GOLDEN, "nw_random.json")) as f:
        pairs = json.load(f)["pairs"]
    for v in pairs:
        o = oracle.nw(v["query"].encode(), v["db"].encode(), literal_dfs=False, scoring=scoring)
        assert (o.score, o.end_states, o.panics, o.n_blocks, o.first_ops) == \
            (v["score"], v["end_states"], v["panics"], v["n_blocks_before_panic"],
             v["first_ops"])
    with open(os.path.join(GOLDEN, "nw_kats.json")) as f:
        data = json.load(f)
    for k in data["hand"]:
        o = oracle.nw(k["query"].encode(), k["db"].encode(), scoring=scoring)
        assert (o.score, o.stdout, o.dfs_rc == 1, o.panics) == \
            (k["score"], k["stdout"], k["panics"], k["panics"]), k["id"]
    o = oracle.nw(b"AAA", b"AA", scoring=scoring)
    for st, arr in (("M", o.M), ("I", o.I), ("D", o.D)):
        assert arr[1:, 1:].tolist() == data["n4_cells"][st], st


def _batch_vs_single(oracle, pairs, s):
    qo = np.zeros(len(pairs) + 1, np.uint64)
    do = np.zeros(len(pairs) + 1, np.uint64)
    qo[1:] = np.cumsum([len(q) for q, _ in pairs])
    do[1:] = np.cumsum([len(d) for _, d in pairs])
    got = oracle.check_pairs(b"".join(q for q, _ in pairs), qo, b"".join(d for _, d in pairs), do,
                             threads=3, scoring=s)
    seen = {"panic": 0, "printed": 0, "dead": 0}
    for k, (q, d) in enumerate(pairs):
        o = oracle.nw(q, d, literal_dfs=False, scoring=s)
        want = (o.score, o.end_states, o.panics, o.first_ops)
        w = got.cigar_words(k)
        first = None if w is None else "".join(OPS[int(x) & 15] * (int(x) >> 4) for x in w)
        assert (int(got.score[k]), int(got.end_states[k]), bool(got.panics[k]), first) == want, \
            (s, k)
        sc, es, pan, lin_first, dead = oracle.nw_first_linear(q, d, threads=2, scoring=s)
        assert (sc, es, pan, lin_first) == want, (s, k)
        assert oracle.nw_score_linear(q, d, 2, scoring=s) == want[:3], (s, k)
        if o.first_ops is not None:
            ps, ok = path_score(q, d, [(1, c) for c in o.first_ops], s)
            assert ok and ps == o.score, (s, k)
        seen["panic"] += o.panics
        seen["printed"] += o.first_ops is not None
        seen["dead"] += dead > 0
    return seen


@pytest.mark.parametrize("scheme", [(2, -3, -5, -2), (1, 0, 0, 0), (8, -8, -16, -12)])
def test_check_pairs_and_linear_match_full_under_schemes(oracle, scheme):
    rng = np.random.default_rng(sum(scheme) & 0xFF)
    pairs = []
    for k in range(100):
        a = [b"ACGT", b"ACGTN", b"AC"][k % 3]
        pairs.append((rand_seq(rng, int(rng.integers(0, 121)), a),
                      rand_seq(rng, int(rng.integers(0, 121)), a)))
    seen = _batch_vs_single(oracle, pairs, scheme)
    assert seen["printed"] > 20 and seen["panic"] > 10, seen


@pytest.mark.parametrize("scheme", [(5, -4, -8, 1), (5, -4, 2, 1), (5, -4, -20, 3), (2, -3, 0, 1)])
def test_check_pairs_and_linear_match_full_under_positive_extend(oracle, scheme):
    """gap_extend > 0: the boundary gains with every column, so unrelated
    pairs end in a panic node; a pair whose db is its query with a few
    substitutions keeps the diagonal ahead and prints."""
    rng = np.random.default_rng(104 + sum(scheme))
    pairs = []
    for k in range(100):
        a = [b"ACGT", b"ACGTN", b"AC"][k % 3]
        q = rand_seq(rng, int(rng.integers(0, 121)), a)
        if k % 2:
            d = bytearray(q)
            for x in rng.integers(0, max(1, len(d)), len(d) // 16):
                d[int(x)] = a[int(rng.integers(len(a)))]
            pairs.append((q, bytes(d)))
        else:
            pairs.append((q, rand_seq(rng, int(rng.integers(0, 121)), a)))
    seen = _batch_vs_single(oracle, pairs, scheme)
    print(scheme, seen)
    # (where a gap gains more than it costs, every DFS reaches a boundary first)
    assert seen["panic"] > 10 and (seen["printed"] > 20 or scheme != (5, -4, -8, 1)), seen


def test_check_pairs_and_linear_match_full_past_the_sentinel(oracle):
    rng = np.random.default_rng(103)
    pairs = []
    for k in range(40):
        a = [b"ACGT", b"AC"][k % 2]
        pairs.append((rand_seq(rng, int(rng.integers(50, 71)), a),
                      rand_seq(rng, int(rng.integers(50, 71)), a)))
    # one short side: every path to the end holds more than 54 gap columns, so
    # the end cell's maximum is sentinel-rooted and the DFS meets dead ends
    for k in range(40):
        a = [b"ACGT", b"AC"][k % 2]
        short, long_ = rand_seq(rng, int(rng.integers(0, 9)), a), \
            rand_seq(rng, int(rng.integers(56, 71)), a)
        pairs.append((short, long_) if k % 4 < 2 else (long_, short))
    seen = _batch_vs_single(oracle, pairs, SENTINEL_SCHEME)
    assert seen["dead"] and 40 <= seen["printed"] < len(pairs), seen
