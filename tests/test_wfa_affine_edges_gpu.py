"""GPU: the corrected gap-affine WFA (wfa_affine_kernels.hip,
wfa_affine_trace_kernels.hip) at the edges its launch decisions have:
a wave that takes several pairs, the three sequence views (2-bit codes in
LDS, bytes in LDS, bytes in HBM), the exact ring-overflow step at both ring
widths, the smallest and largest ring-slot counts, max_score at the optimum,
the i16 / i32 offset switch, the documented CIGAR tie-break and sequence
buffers at odd addresses.

Every comparison is exact.  Penalties come from the Gotoh DP
(oracle/refaffine.c); which pass a pair ends in (or -2) from the plain model
(tests/wfa_affine_model.py), whose ranges depend on the lengths and the
penalties alone; the intended launch path is asserted beforehand through
the host-only geometry query (wfa_affine.plan_geometry).  Both the score
mode and the alignment mode run unless a test says otherwise; every CIGAR
goes through check_cigar against the DP's penalty."""
import numpy as np
import pytest

from wfa_affine_model import check_cigar, m_widths, mixed_pairs, verdict, wfa_align

pytestmark = pytest.mark.gpu

DEFAULT = (4, 2, 6)
SUB = {65: 67, 67: 71, 71: 84, 84: 65}  # a different base


# ------------------------------------------------------------------ helpers
def _dp(saln, oracle, qs, ds, pen=DEFAULT):
    """The DP's penalty of pair (k, k) for every k."""
    q_seq, q_off = saln.pack_csr(qs)
    d_seq, d_off = saln.pack_csr(ds)
    idx = np.arange(len(qs), dtype=np.uint32)
    return oracle.affine_run_pairs(q_seq, q_off, d_seq, d_off, idx, idx, *pen, threads=8).tolist()


def _expected(qs, ds, dp, pen, w1, w2):
    """The engine's scores: the DP's penalty, or -2 where the model says the
    wavefront outgrows both rings."""
    out = []
    for q, d, w in zip(qs, ds, dp):
        out.append(w if verdict(len(q), len(d), pen, w, w1, w2) != -2 else -2)
    return out


def _run_both(saln, qs, ds, want, pen=DEFAULT, dp=None, **kw):
    """Score mode and alignment mode of pairs (k, k) against `want` (the
    expected scores, negative codes included); returns the CigarBatch."""
    wa = saln.wfa_affine
    pairs = [(k, k) for k in range(len(qs))]
    got = wa.wfa_affine_batch(qs, ds, pairs, penalties=pen,
                              max_score=kw.get("max_score", 0)).tolist()
    assert got == want
    res, cig = wa.wfa_affine_align_batch(qs, ds, pairs, penalties=pen, **kw)
    assert res["score"].tolist() == want
    assert not res["status"].any()
    for k, (q, d) in enumerate(zip(qs, ds)):
        assert int(res["cigar_len"][k]) == len(cig.words(k))
        if want[k] < 0:
            assert len(cig.words(k)) == 0, k
        else:
            check_cigar(saln, q, d, cig[k], want[k], pen, dp[k] if dp is not None else want[k])
    return cig


def _words(cig):
    return [cig.words(k).tolist() for k in range(len(cig))]


def _workgroups(geo_pass, n, cus):
    """The persistent grid of a launch of n pairs with this pass's geometry
    (the per-CU count is the host's own, through the geometry query)."""
    return min(n, geo_pass["workgroups_per_cu"] * cus)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _edge(n):
    return b"A", b"A" * n


# --------------------------------------------------------------- wave reuse
@pytest.fixture(scope="module")
def reuse_batch():
    """6,144 pairs of 0..120 bases in random order of kind: i.i.d., mutated,
    two-letter, with N, one side empty - so within any wave's sequence of
    pairs long follow short, N follow pure ACGT and empty follow full."""
    from sequencealigning_amd import synth
    rng = np.random.default_rng(20240)
    qs, ds = [], []
    for k in range(6144):
        kind = int(rng.integers(0, 8))
        lq, ld = int(rng.integers(0, 121)), int(rng.integers(0, 121))
        if kind in (0, 1):    # i.i.d. ACGT
            q, d = synth.random_bases(k, lq).tobytes(), synth.random_bases(k + 7000, ld).tobytes()
        elif kind in (2, 3):  # mutated (long) ACGT
            q = synth.random_bases(k, 60 + lq // 2).tobytes()
            d = synth.mutate(q, 0.1, seed=k)[:120]
        elif kind == 4:       # two letters
            q = bytes(rng.choice([65, 67], lq).astype(np.uint8))
            d = bytes(rng.choice([65, 67], ld).astype(np.uint8))
        elif kind == 5:       # with N
            q = bytes(rng.choice(list(b"ACGTN"), lq).astype(np.uint8))
            d = bytes(rng.choice(list(b"ACGTN"), ld).astype(np.uint8))
        elif kind == 6:       # short
            q, d = synth.random_bases(k, lq % 6).tobytes(), synth.random_bases(k + 1, ld % 6).tobytes()
        else:                 # one side empty
            q = b"" if k & 8 else synth.random_bases(k, lq).tobytes()
            d = synth.random_bases(k, ld).tobytes() if k & 8 else b""
        qs.append(q)
        ds.append(d)
    return qs, ds


def test_wave_reuse_first_pass(saln, oracle, reuse_batch):
    """More pairs than the largest grid (16 workgroups per CU): every wave of
    both kernels takes several pairs and reuses its LDS (ranges, written
    windows, rings, staged sequences).  The words equal those of the same
    pairs in batches of 64, where every wave takes one pair."""
    qs, ds = reuse_batch
    n = len(qs)
    assert n == 6144 > 16 * _cus()
    assert max(map(len, qs + ds)) <= 120 and min(map(len, qs)) == 0
    dp = _dp(saln, oracle, qs, ds)
    cig = _run_both(saln, qs, ds, dp)
    words = _words(cig)
    wa = saln.wfa_affine
    for lo in range(0, n, 64):
        _, c = wa.wfa_affine_align_batch(qs[lo:lo + 64], ds[lo:lo + 64],
                                         [(k, k) for k in range(64)])
        assert _words(c) == words[lo:lo + 64], lo


def _lopsided(seed, n):
    """n pairs that outgrow a 512-diagonal ring: q of 1..8 bases, d of 520..600."""
    rng = np.random.default_rng(seed)
    qs = [bytes(rng.choice(list(b"ACGTN" if k % 3 == 0 else b"ACGT"),
                           int(rng.integers(1, 9))).astype(np.uint8)) for k in range(n)]
    ds = [bytes(rng.choice(list(b"ACGTN" if k % 5 == 0 else b"ACGT"),
                           520 + 8 * int(rng.integers(0, 11))).astype(np.uint8)) for k in range(n)]
    return qs, ds


def test_wave_reuse_second_pass(saln, saln_opt, oracle):
    """1,024 lopsided pairs that all outgrow a 512-diagonal first ring, in one
    trace chunk: the compact kernel runs several blocks, and score pass 2 and
    the second trace fill (launched once per chunk) each have more pairs than
    workgroups, so their waves take several pairs."""
    wa = saln.wfa_affine
    saln_opt("wfa2.w1", 512)
    n = 1024
    qs, ds = _lopsided(515, n)
    geo = wa.plan_geometry([(len(q), len(d)) for q, d in zip(qs, ds)])
    assert [g["ring_width"] for g in geo] == [512, 2048]
    assert n > 512  # the compact kernel: more than two blocks of 256
    # score pass 2 and, the batch being one chunk (below), the second trace fill
    assert n > _workgroups(geo[1], n, _cus())
    dp = _dp(saln, oracle, qs, ds)
    assert all(verdict(len(q), len(d), DEFAULT, w, 512, 2048) == 2 for q, d, w in zip(qs, ds, dp))
    # the whole batch is one chunk of the default budget (1 GiB), so the
    # second trace fill is one launch over all n pairs
    total = sum(wa.trace_bytes(len(q), len(d), w) for q, d, w in zip(qs, ds, dp))
    assert total <= 1 << 30
    _run_both(saln, qs, ds, dp)


def test_second_ring_trace_in_several_chunks(saln, saln_opt, oracle):
    """24 such pairs with a budget of about five pairs' codes per chunk: the
    second-ring fill runs once per chunk; same words as in one chunk."""
    wa = saln.wfa_affine
    saln_opt("wfa2.w1", 512)
    qs, ds = _lopsided(516, 24)
    dp = _dp(saln, oracle, qs, ds)
    sizes = [wa.trace_bytes(len(q), len(d), w) for q, d, w in zip(qs, ds, dp)]
    budget = 5 * max(sizes)
    assert sum(sizes) > 3 * budget
    one = _run_both(saln, qs, ds, dp)
    several = _run_both(saln, qs, ds, dp, trace_budget=budget)
    assert _words(one) == _words(several)


# ----------------------------------------------------------- sequence views
def _phased(items):
    """items: (sequence, 16-byte phase).  The list to pack: every sequence
    preceded by an unreferenced filler that puts its first byte at that phase
    of the packed buffer; returns (list, index of each item's sequence)."""
    out, idx, cur = [], [], 0
    for s, phase in items:
        pad = (phase - cur) % 16
        if pad:
            out.append(b"T" * pad)
            cur += pad
        idx.append(len(out))
        out.append(s)
        cur += len(s)
    return out, idx


@pytest.fixture(scope="module")
def view_set():
    """1,120 pairs: q (70 bases) against q with one substitution at p, for
    every p and every 16-byte phase of q (and, through 3 a + p, of d); then
    every (lq, ld) in 1..20 x 1..20 as prefixes of one sequence.  with_n:
    the same pairs with one N per pair, equal in both sequences and away from
    p.  Returns per variant (queries, dbs, pairs, plain q, plain d, cigars)."""
    from sequencealigning_amd import synth
    base = synth.random_bases(7070, 70)
    shared = synth.random_bases(7171, 20)
    out = {}
    for with_n in (False, True):
        qi, di, cigs = [], [], []
        for p in range(70):
            q = base.copy()
            if with_n:
                q[(p + 35) % 70] = ord("N")
            d = q.copy()
            d[p] = SUB[int(base[p])]
            for a in range(16):
                qi.append((q.tobytes(), a))
                di.append((d.tobytes(), (3 * a + p) % 16))
                cigs.append([(n, op) for n, op in ((p, "="), (1, "X"), (69 - p, "=")) if n])
        s = shared.copy()
        if with_n:
            s[0] = ord("N")
        for lq in range(1, 21):
            for ld in range(1, 21):
                qi.append((s[:lq].tobytes(), (lq + ld) % 16))
                di.append((s[:ld].tobytes(), (5 * lq + ld) % 16))
                gap = [(lq - ld, "I")] if lq > ld else [(ld - lq, "D")] if ld > lq else []
                cigs.append(None if gap else [(lq, "=")])
        queries, qidx = _phased(qi)
        dbs, didx = _phased(di)
        out[with_n] = (queries, dbs, list(zip(qidx, didx)), [s for s, _ in qi], [s for s, _ in di],
                       cigs)
    return out


def _stages(seqcap, lq, ld):
    """(codes fit at any phase, bytes fit): the kernel's rule (include/saln.h)."""
    return (4 * ((15 + lq + 15) // 16 + (15 + ld + 15) // 16 + 4) <= seqcap,
            ((lq + 47) & ~15) + ld + 48 <= seqcap)


@pytest.mark.parametrize("view", ["codes", "bytes", "hbm", "hbm_n"])
def test_sequence_views(saln, saln_opt, oracle, view_set, view):
    wa = saln.wfa_affine
    queries, dbs, pairs, qs, ds, cigs = view_set[view in ("bytes", "hbm_n")]
    if view.startswith("hbm"):
        saln_opt("wfa2.seq_lds", 0)
    lens = [(len(q), len(d)) for q, d in zip(qs, ds)]
    for g in wa.plan_geometry(lens):
        codes, byts = _stages(g["seqcap"], 70, 70)
        assert (codes, byts) == ((False, False) if view.startswith("hbm") else (True, True))
    dp = _dp(saln, oracle, qs, ds)
    assert dp[:1120] == [4] * 1120
    got = wa.wfa_affine_batch(queries, dbs, pairs).tolist()
    assert got == dp
    res, cig = wa.wfa_affine_align_batch(queries, dbs, pairs)
    assert res["score"].tolist() == dp and not res["status"].any()
    for k, (q, d) in enumerate(zip(qs, ds)):
        check_cigar(saln, q, d, cig[k], dp[k], DEFAULT, dp[k])
        if cigs[k] is not None:
            assert cig[k] == cigs[k], k


def test_sequence_views_mixed_in_one_launch(saln, oracle, view_set):
    """A 9,000-base pair with an N beside the small pairs: its bytes (18 KB)
    are not staged while the codes of the batch are, so it reads HBM (the
    long-sequence variant) in the launch where the ACGT pairs read codes."""
    from sequencealigning_amd import synth
    wa = saln.wfa_affine
    queries, dbs, pairs, qs, ds, cigs = view_set[False]
    big = synth.random_bases(9090, 9000)
    big[4000] = ord("N")
    bd = big.copy()
    at = [3, 4500, 8997]
    for p in at:
        bd[p] = SUB[int(big[p])]
    queries, dbs = queries + [big.tobytes()], dbs + [bd.tobytes()]
    pairs = pairs + [(len(queries) - 1, len(dbs) - 1)]
    for g in wa.plan_geometry([(len(q), len(d)) for q, d in zip(qs, ds)] + [(9000, 9000)]):
        assert _stages(g["seqcap"], 9000, 9000) == (True, False)
    dp = _dp(saln, oracle, qs, ds) + [12]
    assert wa.wfa_affine_batch(queries, dbs, pairs).tolist() == dp
    res, cig = wa.wfa_affine_align_batch(queries, dbs, pairs)
    assert res["score"].tolist() == dp and not res["status"].any()
    for k in range(len(qs)):
        if cigs[k] is not None:
            assert cig[k] == cigs[k], k
    assert cig[len(qs)] == [(3, "="), (1, "X"), (4496, "="), (1, "X"), (4496, "="), (1, "X"),
                            (2, "=")]


# --------------------------------------------------------------- ring edges
def _ring_edge_pairs():
    rng = np.random.default_rng(30600)
    lop_q = bytes(rng.choice(list(b"ACGTN"), 30).astype(np.uint8))
    lop_d = bytes(rng.choice(list(b"ACGTN"), 600).astype(np.uint8))
    ns = [511, 512, 1023, 1024, 2047, 2048]
    return [b"A"] * len(ns) + [lop_q], [b"A" * n for n in ns] + [lop_d], ns


@pytest.mark.parametrize("pen,w1,w2,table", [
    (DEFAULT, 0, 0, {1023: 1, 1024: 2, 2047: 2, 2048: -2}),
    ((1, 0, 1), 512, 1024, {511: 1, 512: 2, 1023: 2, 1024: -2}),
])
def test_ring_overflow_edges(saln, saln_opt, oracle, pen, w1, w2, table):
    """q = A, d = A * n: the wavefront is n + 1 diagonals wide on the step
    that converges, so n = W - 1 is the last pair a ring of W holds and
    n = W overflows on the convergence step.  The same pairs traced by the
    first ring and by the second give the same words."""
    wa = saln.wfa_affine
    qs, ds, ns = _ring_edge_pairs()
    lens = [(len(q), len(d)) for q, d in zip(qs, ds)]
    dp = _dp(saln, oracle, qs, ds, pen)
    geo = wa.plan_geometry(lens, pen)
    assert [g["ring_width"] for g in geo] == [1024, 2048] and not geo[0]["i32_offsets"]
    other = {}  # the other pair of ring widths: the first table's under w1 = 512
    if w1:
        other = _run_both(saln, qs, ds, _expected(qs, ds, dp, pen, 1024, 2048), pen, dp)
        saln_opt("wfa2.w1", w1)
        saln_opt("wfa2.w2", w2)
        geo = wa.plan_geometry(lens, pen)
    W1, W2 = (g["ring_width"] for g in geo)
    assert (W1, W2) == (w1 or 1024, w2 or 2048)
    for n, v in table.items():
        k = ns.index(n)
        assert verdict(1, n, pen, dp[k], W1, W2) == v, n
        assert max(m_widths(1, n, pen, dp[k])) == n + 1
    want = _expected(qs, ds, dp, pen, W1, W2)
    assert [want[ns.index(n)] < 0 for n in table] == [v == -2 for v in table.values()]
    cig = _run_both(saln, qs, ds, want, pen, dp)
    if not w1:
        saln_opt("wfa2.w1", 512)
        other = _run_both(saln, qs, ds, _expected(qs, ds, dp, pen, 512, 2048), pen, dp)
    n_same = 0
    for k in range(len(qs)):
        a, b = cig.words(k).tolist(), other.words(k).tolist()
        if a and b:
            assert a == b, k
            n_same += 1
    assert n_same >= 4


# --------------------------------------------------------------- ring slots
@pytest.fixture(scope="module")
def small_mixed():
    qs, ds = mixed_pairs(23, n=60, max_len=160)
    assert len(qs) == 64 and max(map(len, qs + ds)) <= 200
    return qs, ds


@pytest.mark.parametrize("pen,slots,widths", [
    ((1, 0, 1), (2, 2), (1024, 2048)),       # the fewest slots
    ((15, 14, 1), (16, 2), (1024, 1024)),    # the most M slots; second ring narrowed
    ((7, 11, 1), (13, 2), (1024, 1024)),     # second ring narrowed (70,400 bytes at 2048)
    ((6, 5, 3), (9, 4), (1024, 1024)),
])
def test_ring_slot_counts(saln, oracle, small_mixed, pen, slots, widths):
    from math import gcd
    wa = saln.wfa_affine
    x, o, e = pen
    g = gcd(gcd(x, o + e), e)
    assert (max(x, o + e) // g + 1, e // g + 1) == slots
    qs, ds = list(small_mixed[0]), list(small_mixed[1])
    if pen == (1, 0, 1):
        # a wavefront above 256 diagonals: the second group of the branch-free loop
        from sequencealigning_amd import synth
        qs.append(synth.random_bases(3001, 300).tobytes())
        ds.append(synth.random_bases(3002, 300).tobytes())
    geo = wa.plan_geometry([(len(q), len(d)) for q, d in zip(qs, ds)], pen)
    assert tuple(p["ring_width"] for p in geo) == widths
    assert all(p["lds_bytes"] <= 65536 for p in geo)
    dp = _dp(saln, oracle, qs, ds, pen)
    if pen == (1, 0, 1):
        assert max(m_widths(300, 300, pen, dp[-1])) > 256
    _run_both(saln, qs, ds, _expected(qs, ds, dp, pen, *widths), pen, dp)


# ---------------------------------------------------------------- max_score
@pytest.mark.parametrize("pen", [DEFAULT, (1, 3, 1)])
def test_max_score_at_the_optimum(saln, oracle, pen):
    """The score is returned iff it is <= max_score - at the optimum itself,
    one below (odd under (4,2,6), where scores step by g = 2) and one above;
    pairs with an empty side follow the same rule."""
    wa = saln.wfa_affine
    qs, ds = mixed_pairs(31, n=12, max_len=80)
    assert len(qs) == 16
    pairs = [(k, k) for k in range(16)]
    dp = _dp(saln, oracle, qs, ds, pen)
    caps = sorted({c for w in dp for c in (w - 1, w, w + 1) if c > 0})
    if pen == DEFAULT:
        assert all(w % 2 == 0 for w in dp) and any(c % 2 for c in caps)
    for cap in caps:
        want = [w if w <= cap else -1 for w in dp]
        assert wa.wfa_affine_batch(qs, ds, pairs, penalties=pen, max_score=cap).tolist() == want, cap
        res, cig = wa.wfa_affine_align_batch(qs, ds, pairs, penalties=pen, max_score=cap)
        assert res["score"].tolist() == want and not res["status"].any(), cap
        for k in range(16):
            if want[k] < 0:
                assert len(cig.words(k)) == 0
            else:
                check_cigar(saln, qs[k], ds[k], cig[k], want[k], pen, dp[k])


# ------------------------------------------------------------- offset types
@pytest.mark.parametrize("n,wide", [(32000, False), (32001, True)])
def test_offset_type_switch(saln, n, wide):
    """32,000 bases run i16 offsets, 32,001 i32.  Three substitutions in the
    last 100 bases score 12 (a gapped alignment of equal lengths costs at
    least 2 (o + e) = 16); one base deleted near the end scores o + e = 8."""
    from sequencealigning_amd import synth
    wa = saln.wfa_affine
    q = synth.random_bases(3200 + n, n)
    d_sub = q.copy()
    at = [n - 90, n - 40, n - 2]
    for p in at:
        d_sub[p] = SUB[int(q[p])]
    cut = n - 50
    while q[cut] == q[cut - 1] or q[cut] == q[cut + 1]:
        cut -= 1  # a deleted base that differs from its neighbours: one place for the gap
    d_del = np.delete(q, cut)
    qs = [q.tobytes(), q.tobytes()]
    ds = [d_sub.tobytes(), d_del.tobytes()]
    geo = wa.plan_geometry([(len(a), len(b)) for a, b in zip(qs, ds)])
    assert [g["i32_offsets"] for g in geo] == [wide, wide]
    assert [g["ring_width"] for g in geo] == ([512, 1024] if wide else [1024, 2048])
    cig = _run_both(saln, qs, ds, [12, 8])
    assert cig[0] == [(n - 90, "="), (1, "X"), (49, "="), (1, "X"), (37, "="), (1, "X"), (1, "=")]
    assert cig[1] == [(cut, "="), (1, "I"), (n - 1 - cut, "=")]


@pytest.mark.parametrize("pen", [DEFAULT, (1, 3, 1)])
def test_wide_plan_batch(saln, oracle, small_mixed, pen):
    """One identical 32,001-base pair (score 0) makes the plan wide: the
    small pairs and the ring-edge pairs then run the i32 kernels with rings
    of 512 and 1,024 diagonals - the narrow score path, the i32 rerun and
    the i32 trace."""
    from sequencealigning_amd import synth
    wa = saln.wfa_affine
    long = synth.random_bases(32001, 32001).tobytes()
    ns = [511, 512, 1023, 1024]
    qs = [long] + [b"A"] * 4 + list(small_mixed[0])
    ds = [long] + [b"A" * n for n in ns] + list(small_mixed[1])
    geo = wa.plan_geometry([(len(q), len(d)) for q, d in zip(qs, ds)], pen)
    assert [g["ring_width"] for g in geo] == [512, 1024]
    assert all(g["i32_offsets"] and g["lds_bytes"] <= 65536 for g in geo)
    dp = [0] + _dp(saln, oracle, qs[1:], ds[1:], pen)
    want = _expected(qs, ds, dp, pen, 512, 1024)
    v = [verdict(1, n, pen, dp[1 + i], 512, 1024) for i, n in enumerate(ns)]
    if pen == DEFAULT:
        assert v == [1, 2, 2, -2] and want[1:5] == dp[1:4] + [-2]
    assert 2 in v and -2 in v
    cig = _run_both(saln, qs, ds, want, pen, dp)
    assert cig[0] == [(32001, "=")]


# ---------------------------------------------------------------- tie-break
@pytest.fixture(scope="module")
def tie_pairs():
    rng = np.random.default_rng(1207)
    qs, ds = [], []
    for k in range(200):
        lq, ld = int(rng.integers(1, 121)), int(rng.integers(1, 121))
        if k % 4 == 3:      # four letters, with N
            al = list(b"ACGTN")
        elif k % 4 == 2:    # one letter with rare breaks
            al = [65] * 7 + [67]
        else:               # two letters
            al = [65, 67]
        q = bytes(rng.choice(al, lq).astype(np.uint8))
        if k % 8 < 2:       # a mutated copy: runs of '=' between the edits
            d = bytearray(q)
            for _ in range(int(rng.integers(1, 6))):
                p = int(rng.integers(0, len(d) + 1))
                if rng.integers(0, 2) and p < len(d):
                    del d[p]
                else:
                    d.insert(p, int(rng.choice(al)))
            d = bytes(d[:120]) or b"A"
        else:
            d = bytes(rng.choice(al, ld).astype(np.uint8))
        qs.append(q)
        ds.append(d)
    return qs, ds


@pytest.mark.parametrize("pen", [DEFAULT, (1, 0, 1), (3, 5, 1)])
def test_tie_break_is_the_documented_one(saln, oracle, tie_pairs, pen):
    """The engine's CIGAR equals the model's word for word: M prefers the
    mismatch, then the db-advancing gap ('D'), then the query-advancing gap
    ('I'); a gap prefers extend over open (include/saln.h).  Scores (both
    modes) and CIGARs are held to the DP as everywhere."""
    qs, ds = tie_pairs
    assert len(qs) == 200 and max(map(len, qs + ds)) <= 120
    dp = _dp(saln, oracle, qs, ds, pen)
    cig = _run_both(saln, qs, ds, dp, pen)
    n_gapped = 0
    for k, (q, d) in enumerate(zip(qs, ds)):
        score, _, want = wfa_align(q, d, pen)
        assert score == dp[k], k
        assert cig[k] == want, (k, q, d)
        n_gapped += any(op in "ID" for _, op in want)
    assert n_gapped > 100


# ------------------------------------------------------ device plan, odd bases
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_device_plan_at_odd_alignments(saln, saln_opt, oracle, small_mixed, shift):
    """WfaAffinePlan.execute on sequence buffers that start 1, 7 and 15 bytes
    into a larger tensor (16 readable bytes after the last base), staged and
    from HBM.  Score mode (the plan has no alignment mode)."""
    import torch
    qs, ds = small_mixed
    n = len(qs)
    q_seq, q_off = saln.pack_csr(qs)
    d_seq, d_off = saln.pack_csr(ds)
    want = _dp(saln, oracle, qs, ds)
    hq = np.full(shift + len(q_seq) + 16, ord("T"), np.uint8)
    hd = np.full(16 - shift + len(d_seq) + 16, ord("T"), np.uint8)
    hq[shift:shift + len(q_seq)] = q_seq
    hd[16 - shift:16 - shift + len(d_seq)] = d_seq
    dq, dd = torch.from_numpy(hq).cuda(), torch.from_numpy(hd).cuda()
    assert dq.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
    for seq_lds in (24 * 1024, 0):
        saln_opt("wfa2.seq_lds", seq_lds)
        plan = saln.wfa_affine.WfaAffinePlan(q_off, d_off, [(k, k) for k in range(n)])
        sc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        plan.execute(dq[shift:], dd[16 - shift:], sc)
        torch.cuda.synchronize()
        assert sc.cpu().tolist() == want, seq_lds
        plan.close()


# ------------------------------------------------------- refused ring widths
def test_unsupported_ring_width_never_launches(saln, saln_opt):
    """A ring width the kernels cannot run is refused by the plan's host
    logic, before any device call (the CPU tests pin the decision itself)."""
    from sequencealigning_amd import _lib
    wa = saln.wfa_affine
    for name, v in (("wfa2.w1", 256), ("wfa2.w2", 4096), ("wfa2.w1", 1000)):
        saln_opt(name, v)
        with pytest.raises(_lib.SalnError, match="E_INVALID"):
            wa.wfa_affine_batch([b"ACGT"], [b"ACGA"])
        with pytest.raises(_lib.SalnError, match="E_INVALID"):
            wa.wfa_affine_align_batch([b"ACGT"], [b"ACGA"])
        saln_opt(name, 0)
    assert wa.wfa_affine(b"ACGT", b"ACGA") == 4
