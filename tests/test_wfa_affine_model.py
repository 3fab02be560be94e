"""CPU: the plain WFA model of the corrected-WFA GPU tests
(tests/wfa_affine_model.py) held to the existing oracle, its range part at
the fixed ring-edge cases, and the host-only launch geometry
(saln_wfa_affine_plan_geometry): no pass above 65,536 bytes of LDS for any
accepted penalty set, and only ring widths the kernels run."""
from math import gcd

import pytest

from wfa_affine_model import check_cigar, m_widths, mixed_pairs, verdict, wfa_align

PENS = [(4, 2, 6), (1, 3, 1), (5, 0, 2), (3, 5, 1), (1, 0, 1), (15, 14, 1)]
LDS_LIMIT = 65536


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
@pytest.mark.parametrize("pen", PENS)
def test_model_matches_dp(saln, oracle, pen, seed):
    """Penalty = the Gotoh DP's; the CIGAR passes the shared checker; the
    widths cover exactly the steps up to the penalty.  Four seeds of 66 drawn
    pairs (264 per penalty set, plus the fixed empty / identical ones), no
    sequence above 150 bases."""
    qs, ds = mixed_pairs(seed, n=66, max_len=120)
    assert len(qs) == len(ds) == 70 and max(map(len, qs + ds)) <= 150
    g = gcd(gcd(pen[0], pen[1] + pen[2]), pen[2])
    for q, d in zip(qs, ds):
        want = oracle.affine_penalty(q, d, *pen)
        score, widths, cigar = wfa_align(q, d, pen)
        assert score == want, (q, d)
        check_cigar(saln, q, d, cigar, score, pen, want)
        if q and d:
            assert widths == m_widths(len(q), len(d), pen, want)
            assert len(widths) == want // g
            assert max(widths, default=1) <= len(q) + len(d) + 1


def test_model_tie_break_by_hand():
    """Small cases worked by hand from the documented tie-break."""
    # one substitution or one gap pair? x = 4 < 2 (o + e) = 16: the mismatch
    # (g = 2: step 1 is score 2, which no cell has; step 2 is the diagonal)
    assert wfa_align(b"ACGT", b"AGGT", (4, 2, 6)) == (4, [0, 1], [(1, "="), (1, "X"), (2, "=")])
    # AA vs A: the gap can sit in either column at cost o + e; the M entry of
    # the last step comes from D (query-advancing, 'I'), opened from M[0][0]
    # after its extension over the first column: the gap is the last column
    assert wfa_align(b"AA", b"A", (4, 2, 6))[::2] == (8, [(1, "="), (1, "I")])
    assert wfa_align(b"A", b"AA", (4, 2, 6))[::2] == (8, [(1, "="), (1, "D")])
    # CA vs AC under (1,0,1): X X (2) ties with D..I (2); M prefers the mismatch
    assert wfa_align(b"CA", b"AC", (1, 0, 1))[::2] == (2, [(2, "X")])
    # empty sides: one gap run, query first
    assert wfa_align(b"", b"ACG", (4, 2, 6)) == (20, [], [(3, "D")])
    assert wfa_align(b"AC", b"", (1, 3, 1)) == (5, [], [(2, "I")])
    assert wfa_align(b"", b"", (4, 2, 6)) == (0, [], [])


@pytest.mark.parametrize("W", [512, 1024, 2048])
@pytest.mark.parametrize("pen,optimum", [((4, 2, 6), lambda n: 6 * n - 4),
                                         ((1, 0, 1), lambda n: n - 1)])
def test_ring_edge_widths(oracle, pen, optimum, W):
    """q = A, d = A * n: the optimum, the width n + 1 at the final step
    (and nowhere wider), so n = W - 1 fits a ring of W and n = W overflows
    on the convergence step."""
    for n in (W - 1, W):
        w = optimum(n)
        if W == 512:
            assert oracle.affine_penalty(b"A", b"A" * n, *pen) == w
        widths = m_widths(1, n, pen, w)
        assert widths[-1] == n + 1 == max(widths)
        assert max(widths[:-1]) <= n
    assert verdict(1, W - 1, pen, optimum(W - 1), W, 2 * W) == 1
    assert verdict(1, W, pen, optimum(W), W, 2 * W) == 2
    assert verdict(1, W, pen, optimum(W), W // 2, W) == -2
    # the small model agrees with the closed form where it is cheap
    score, widths, cigar = wfa_align(b"A", b"A" * 40, pen)
    assert score == optimum(40) and widths[-1] == 41
    assert sorted(cigar) == [(1, "="), (39, "D")]


# ------------------------------------------------------------ geometry query
def _accepted(x, o, e):
    g = gcd(gcd(x, o + e), e)
    return max(x, o + e) // g + 1 <= 16 and e // g + 1 <= 16


def _ring_bytes(pen, W, wide):
    x, o, e = pen
    g = gcd(gcd(x, o + e), e)
    return 768 + (max(x, o + e) // g + 1 + 2 * (e // g + 1)) * W * (4 if wide else 2)


def test_geometry_every_accepted_penalty_fits_lds(saln):
    """x, e in 1..16, o in 0..16, both offset types: each pass asks for at
    most 65,536 bytes, at the widest supported ring that fits; a set whose
    rings do not fit at 512 is refused."""
    wa = saln.wfa_affine
    from sequencealigning_amd._lib import SalnError
    n_ok = n_refused = n_clamped = 0
    for wide in (False, True):
        lens = [(100, 120), (32001 if wide else 32000, 50)]
        defaults = (512, 1024) if wide else (1024, 2048)
        for x in range(1, 17):
            for o in range(0, 17):
                for e in range(1, 17):
                    pen = (x, o, e)
                    if not _accepted(*pen):
                        with pytest.raises(SalnError, match="E_INVALID"):
                            wa.plan_geometry(lens, pen)
                        continue
                    if _ring_bytes(pen, 512, wide) > LDS_LIMIT:
                        with pytest.raises(SalnError, match=f"\\({x}, {o}, {e}\\)"):
                            wa.plan_geometry(lens, pen)
                        n_refused += 1
                        continue
                    geo = wa.plan_geometry(lens, pen)
                    for p, dflt in zip(geo, defaults):
                        want_w = max(w for w in (512, 1024, 2048)
                                     if w <= dflt and (w == 512 or _ring_bytes(pen, w, wide) <= LDS_LIMIT))
                        assert p["ring_width"] == want_w, (pen, wide, p)
                        assert p["lds_bytes"] <= LDS_LIMIT, (pen, wide, p)
                        assert p["lds_bytes"] == _ring_bytes(pen, want_w, wide) + p["seqcap"]
                        assert p["seqcap"] >= 0 and p["i32_offsets"] == wide
                        assert 1 <= p["workgroups_per_cu"] <= 16
                        assert p["workgroups_per_cu"] * p["lds_bytes"] <= 160 << 10
                        n_clamped += want_w != dflt
                    n_ok += 1
    assert n_ok > 1000 and n_clamped > 0
    assert n_refused > 0  # i32 offsets with 16 + 2 * 16 slots: 99,072 bytes at 512


def test_geometry_defaults_and_clamp(saln, saln_opt):
    wa = saln.wfa_affine
    small = [(100, 120)]
    g = wa.plan_geometry(small)
    assert [p["ring_width"] for p in g] == [1024, 2048]
    assert [p["i32_offsets"] for p in g] == [False, False]
    assert g[0]["lds_bytes"] - g[0]["seqcap"] == 768 + 13 * 1024 * 2
    assert g[1]["lds_bytes"] - g[1]["seqcap"] == 54016
    # as many one-wave workgroups per CU as 160 KB of LDS hold, at most 16
    assert [p["workgroups_per_cu"] for p in g] == [5, 3]
    assert [p["workgroups_per_cu"] for p in wa.plan_geometry(small, (1, 0, 1))] == [12, 6]
    assert [p["workgroups_per_cu"] for p in wa.plan_geometry([(3, 3)], (1, 0, 1))] == [12, 6]
    g = wa.plan_geometry(small + [(32001, 32001)])
    assert [p["ring_width"] for p in g] == [512, 1024]
    assert [p["i32_offsets"] for p in g] == [True, True]
    # seqcap never exceeds what the rings leave, whatever wfa2.seq_lds asks
    for seq_lds in (0, 100, 8192, 24 * 1024, 64 * 1024):
        saln_opt("wfa2.seq_lds", seq_lds)
        for lens in (small, [(3000, 3000)], [(32000, 32000)], [(32001, 32001)], [(10 ** 6, 5)]):
            for pen in ((4, 2, 6), (7, 11, 1), (15, 14, 1), (1, 0, 15)):
                if pen == (1, 0, 15) and max(lens[0]) > 32000:
                    continue  # 48 slots of i32 offsets: refused (the sweep above)
                for p in wa.plan_geometry(lens, pen):
                    rings = p["lds_bytes"] - p["seqcap"]
                    assert 0 <= p["seqcap"] <= LDS_LIMIT - rings, (seq_lds, lens, pen, p)
                    assert p["seqcap"] <= ((seq_lds + 15) & ~15)
    saln_opt("wfa2.seq_lds", 0)
    assert [p["seqcap"] for p in wa.plan_geometry(small)] == [0, 0]
    saln_opt("wfa2.seq_lds", 24 * 1024)
    # (7,11,1) and (6,5,3): 70,400 bytes at 2048 - the second pass is narrowed
    for pen in ((7, 11, 1), (6, 5, 3)):
        g = wa.plan_geometry(small, pen)
        assert [p["ring_width"] for p in g] == [1024, 1024]
    assert [p["ring_width"] for p in wa.plan_geometry(small, (15, 14, 1))] == [1024, 1024]
    assert [p["ring_width"] for p in wa.plan_geometry(small, (1, 0, 15))] == [512, 512]
    # a requested width is narrowed the same way
    saln_opt("wfa2.w1", 2048)
    assert [p["ring_width"] for p in wa.plan_geometry(small, (1, 0, 15))] == [512, 512]
    assert [p["ring_width"] for p in wa.plan_geometry(small)] == [2048, 2048]


@pytest.mark.parametrize("name", ["wfa2.w1", "wfa2.w2"])
def test_geometry_refuses_unsupported_ring_widths(saln, saln_opt, name):
    """The option stores 0..4096; the engine runs 0 (default), 512, 1024 and
    2048 only and refuses the plan otherwise (include/saln.h)."""
    wa = saln.wfa_affine
    from sequencealigning_amd import _lib
    for v in (512, 1024, 2048, 0):
        saln_opt(name, v)
        wa.plan_geometry([(10, 10)])
    for v in (1, 64, 255, 256, 500, 513, 1000, 1536, 2047, 3000, 4096):
        saln_opt(name, v)
        with pytest.raises(_lib.SalnError, match="E_INVALID.*" + name.replace(".", r"\.")):
            wa.plan_geometry([(10, 10)])
    with pytest.raises(_lib.SalnError, match="E_INVALID"):
        _lib.set_option(name, 4097)
    with pytest.raises(_lib.SalnError, match="E_INVALID"):
        _lib.set_option(name, -1)
