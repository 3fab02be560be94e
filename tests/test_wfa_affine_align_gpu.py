"""GPU: the alignment mode of the corrected gap-affine WFA
(wfa_affine_trace_kernels.hip through saln_wfa_affine_align_batch).  Every
CIGAR goes through one checker: run-length maximal, consumes both sequences
exactly, '=' columns equal and 'X' columns different, and its gap-affine
penalty equals both the returned score and the Gotoh DP's minimum
(oracle/refaffine.c)."""
import pytest

from wfa_affine_model import check_cigar, mixed_pairs

pytestmark = pytest.mark.gpu

PENS = [(4, 2, 6), (1, 3, 1), (5, 0, 2), (3, 5, 1)]


def _pairs(seed):
    """96 mixed pairs of up to 400 (db: 500) bases and four fixed ones."""
    return mixed_pairs(seed)


@pytest.fixture(scope="module")
def mixed():
    return _pairs(7)


@pytest.fixture(scope="module")
def mixed_dp(oracle, mixed):
    """The DP's penalties of the mixed pairs, once per penalty set."""
    qs, ds = mixed
    return {pen: [oracle.affine_penalty(q, d, *pen) for q, d in zip(qs, ds)] for pen in PENS}


@pytest.mark.parametrize("pen", PENS)
def test_align_mixed_small_pairs(saln, mixed, mixed_dp, pen):
    qs, ds = mixed
    res, cig = saln.wfa_affine.wfa_affine_align_batch(
        qs, ds, [(k, k) for k in range(len(qs))], penalties=pen)
    assert len(res) == len(cig) == 100
    for k, (q, d) in enumerate(zip(qs, ds)):
        assert int(res["status"][k]) == 0, k
        assert int(res["cigar_len"][k]) == len(cig[k])
        check_cigar(saln, q, d, cig[k], int(res["score"][k]), pen, mixed_dp[pen][k])
    # the pairs with an empty side: one gap run, or no words
    assert cig[96] == [] and cig[97] == [(1, "I")] and cig[98] == [(3, "D")]
    assert cig[99] == [(4, "=")]


def test_align_both_ring_widths(saln, oracle):
    from sequencealigning_amd import synth
    wa = saln.wfa_affine
    q0 = synth.random_bases(900, 2000).tobytes()
    qs = [q0, synth.random_bases(990, 1500).tobytes(), synth.random_bases(990, 3000).tobytes()]
    ds = [synth.mutate(q0, 0.05, seed=950), synth.random_bases(991, 1300).tobytes(),
          synth.random_bases(991, 2500).tobytes()]
    pairs = [(k, k) for k in range(3)]
    plain = wa.wfa_affine_batch(qs, ds, pairs).tolist()
    assert plain[0] == 540 == oracle.affine_penalty(qs[0], ds[0])
    assert plain[1] == 3888 == oracle.affine_penalty(qs[1], ds[1])  # second ring, not -2
    res, cig = wa.wfa_affine_align_batch(qs, ds, pairs)
    assert res["score"].tolist() == plain
    assert res["status"].tolist() == [0, 0, 0]
    for k in range(2):
        check_cigar(saln, qs[k], ds[k], cig[k], int(res["score"][k]), (4, 2, 6), plain[k])
    # past the widest ring: what the score pass says (-2 expected), no words
    if plain[2] < 0:
        assert int(res["cigar_len"][2]) == 0 and cig[2] == []
    else:
        check_cigar(saln, qs[2], ds[2], cig[2], plain[2], (4, 2, 6), 7816)


def test_align_all_vs_all_and_cap(saln, oracle):
    from sequencealigning_amd import synth
    qs = [synth.random_bases(10 + k, 50 + 13 * k).tobytes() for k in range(5)]
    ds = [synth.mutate(qs[k % 5], 0.1, seed=k) for k in range(4)]
    order = [(q, d) for d in ds for q in qs]  # db outer, query inner
    want = [oracle.affine_penalty(q, d) for q, d in order]
    res, cig = saln.wfa_affine.wfa_affine_align_batch(qs, ds)
    assert res["score"].tolist() == want
    for k, (q, d) in enumerate(order):
        check_cigar(saln, q, d, cig[k], want[k], (4, 2, 6), want[k])
    res, cig = saln.wfa_affine.wfa_affine_align_batch(qs, ds, max_score=60)
    assert any(w > 60 for w in want) and any(w <= 60 for w in want)
    for k, (q, d) in enumerate(order):
        assert int(res["status"][k]) == 0
        if want[k] > 60:
            assert int(res["score"][k]) == -1 and cig[k] == []
        else:
            check_cigar(saln, q, d, cig[k], int(res["score"][k]), (4, 2, 6), want[k])


def _words(cig):
    return [cig.words(k).tolist() for k in range(len(cig))]


def test_align_chunking_and_trace_cap(saln, mixed, mixed_dp):
    wa = saln.wfa_affine
    qs, ds = mixed[0][:32], mixed[1][:32]
    pairs = [(k, k) for k in range(32)]
    want = mixed_dp[(4, 2, 6)][:32]
    sizes = [wa.trace_bytes(len(q), len(d), w) for q, d, w in zip(qs, ds, want)]
    big = max(sizes)
    assert sum(sizes) > 2 * big  # several chunks below
    res1, cig1 = wa.wfa_affine_align_batch(qs, ds, pairs)
    assert res1["score"].tolist() == want and not res1["status"].any()
    res2, cig2 = wa.wfa_affine_align_batch(qs, ds, pairs, trace_budget=big + 1)
    assert (res1 == res2).all()
    assert _words(cig1) == _words(cig2)
    res3, cig3 = wa.wfa_affine_align_batch(qs, ds, pairs, trace_budget=big - 1)
    for k in range(32):
        if sizes[k] == big:
            assert (int(res3["score"][k]), int(res3["status"][k]),
                    int(res3["cigar_len"][k])) == (want[k], wa.TRACE_CAP, 0)
            assert cig3[k] == []
        else:
            assert res3[k] == res1[k]
            assert cig3.words(k).tolist() == cig1.words(k).tolist()


def test_align_deterministic(saln, mixed):
    wa = saln.wfa_affine
    qs, ds = mixed
    n = len(qs)
    fwd = [(k, k) for k in range(n)]
    res1, cig1 = wa.wfa_affine_align_batch(qs, ds, fwd)
    res2, cig2 = wa.wfa_affine_align_batch(qs, ds, fwd)
    res3, cig3 = wa.wfa_affine_align_batch(qs, ds, fwd[::-1])
    assert (res1 == res2).all() and (res1 == res3[::-1]).all()
    w1 = _words(cig1)
    assert w1 == _words(cig2)
    assert w1 == _words(cig3)[::-1]


def test_align_i32_offsets(saln):
    """33,000 bases: the i32-offset kernels.  12 substitutions at least 1,000
    bases apart: the alignment is 12 'X' columns and no gap; the score is
    the score-only path's (pinned to the DP elsewhere)."""
    from sequencealigning_amd import synth
    wa = saln.wfa_affine
    q = synth.random_bases(3300, 33_000)
    d = q.copy()
    sub = {65: 67, 67: 71, 71: 84, 84: 65}
    at = [1500 + 2500 * i for i in range(12)]
    for p in at:
        d[p] = sub[int(d[p])]
    q, d = q.tobytes(), d.tobytes()
    plain = int(wa.wfa_affine_batch([q], [d], [(0, 0)])[0])
    score, cigar = wa.wfa_affine_align(q, d)
    assert score == plain == 48
    check_cigar(saln, q, d, cigar, score, (4, 2, 6))
    assert [op for _, op in cigar if op != "="] == ["X"] * 12
    assert sum(n for n, op in cigar if op == "X") == 12
