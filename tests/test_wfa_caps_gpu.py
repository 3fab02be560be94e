"""GPU: the reference-semantics WFA engine (wfa_kernels.hip, wfa_host.cpp) at
its edges, against the oracle (oracle/refwfa.c) through wfa_check: the width
cap, the boundary between the short first pass and the re-run pass, launches
in several chunks, and the four-bytes-at-a-time extension.  Every case runs
the three host entries: saln_wfa_render_batch (one pass, with logs),
saln_wfa_align_batch (two passes) and saln_wfa_plan_* (device buffers).

The traceback's movement branches have no test here: no input reaches them
(test_wfa_caps.py::test_traceback_never_moves)."""
import numpy as np
import pytest

from wfa_check import NONCONVERGED, expected, seeded_pairs, width_cap_step, widths

pytestmark = pytest.mark.gpu

FIELDS = ("score", "status", "steps", "conv_offset", "conv_state", "conv_np")
A21 = (b"A" * 21, b"C")


def _plan_run(saln, qs, ds, pairs, kw, shift=(0, 0), executes=1):
    """saln_wfa_plan_* on device copies of the CSR bytes that start `shift`
    bytes into their (zero-padded) buffers; one result array per execute."""
    import torch
    q_seq, q_off = saln.pack_csr(qs)
    d_seq, d_off = saln.pack_csr(ds)

    def dev(a, sh):
        buf = torch.zeros(len(a) + sh + 8, dtype=torch.uint8, device="cuda")
        buf[sh:sh + len(a)] = torch.from_numpy(a.copy()).cuda()
        return buf[sh:]

    dq, dd = dev(q_seq, shift[0]), dev(d_seq, shift[1])
    plan = saln.WfaPlan(q_off, d_off, pairs=pairs, **kw)
    got = []
    try:
        for _ in range(executes):
            out = torch.full((len(pairs) * 8,), -1, dtype=torch.int32, device="cuda")
            plan.execute(dq, dd, out)
            torch.cuda.synchronize()
            got.append(out.cpu().numpy().view(saln._lib.WFA_RESULT_DTYPE))
    finally:
        plan.close()
    return got


def _paths(saln, qs, ds, max_steps, max_width=None, pairs=None, shift=(0, 0)):
    """(texts, {path: results}) of the pairs (default: k-th with k-th)."""
    if pairs is None:
        pairs = [(k, k) for k in range(len(qs))]
    kw = {"max_steps": max_steps}
    if max_width is not None:
        kw["max_width"] = max_width
    texts, rres = saln.wfa.render_batch(qs, ds, pairs, with_results=True, **kw)
    bres, _ = saln.wfa_align_batch(qs, ds, pairs=pairs, **kw)
    pres, = _plan_run(saln, qs, ds, pairs, kw, shift)
    return texts, {"render": rres, "batch": bres, "plan": pres}


def _check_expected(texts, res, exp, tag):
    """Every path gives exp[k]'s status, steps and score; the text matches."""
    for k, e in enumerate(exp):
        for path, r in res.items():
            got = (int(r["status"][k]), int(r["steps"][k]), int(r["score"][k]))
            assert got == (e.status, e.steps, e.score), (tag, path, k)
        assert texts[k] == (e.stdout, e.status), (tag, k)


def test_width_cap_edges(saln, oracle):
    """max_width of exactly the widest wavefront of an 80-step run (must not
    bind), one less (must stop the pair at the call that builds that
    wavefront), 7 (stops in the first pass, at call 24 where it binds) and 9
    (stops at call 30 or 36, either side of the first pass's cap)."""
    cases = [A21, (b"ACGT", b"ACGT"), (b"", b"ACG")] + seeded_pairs(31, 30, max_len=24)
    by_width = {}
    for q, d in cases:
        w = max(widths(oracle.wfa(q, d, max_steps=80).stdout), default=0)
        for W in {w, w - 1, 7, 9}:
            if W >= 1:
                by_width.setdefault(W, []).append((q, d, w))
    stops = set()
    for W, lst in sorted(by_width.items()):
        qs, ds = [c[0] for c in lst], [c[1] for c in lst]
        exp = [expected(oracle, q, d, 80, W) for q, d in zip(qs, ds)]
        for (q, d, w), e in zip(lst, exp):
            k = width_cap_step(oracle, q, d, W, 80)
            if W == w:
                assert k is None
            if W == w - 1:
                assert k is not None and (e.status, e.score) == (NONCONVERGED, k)
            if k is not None:
                stops.add(k)
        texts, res = _paths(saln, qs, ds, 80, W)
        _check_expected(texts, res, exp, W)
    assert {24, 30, 36} <= stops and max(stops) > 64, stops


def test_default_width_at_long_caps(saln, oracle):
    """The default width (64) binds beyond 127 steps.  (A*21, C) at a 400-step
    cap stops at call 354; at width 67 at call 372; width 68 never binds.  The
    26 x 9 bp pair is pair 105 of test_two_pass_cap_matches_oracle's
    generator at seed 2: its 184th `lo/hi` line is the first of width 65 and
    is printed by call 374 (the first max_steps at which the oracle prints
    it), where the default width stops it."""
    q, d = A21
    for W, k in ((None, 354), (67, 372), (68, None)):
        assert width_cap_step(oracle, q, d, W or 64, 400) == k
        texts, res = _paths(saln, [q], [d], 400, W)
        _check_expected(texts, res, [expected(oracle, q, d, 400, W or 64)], W)
        for r in res.values():
            assert int(r["steps"][0]) == (k or 400) and int(r["status"][0]) == NONCONVERGED
            assert int(r["score"][0]) == (k or 401)
    q, d = b"CTTGTGATATGAAGATAGTGGTGGCC", b"GCCGCGCTG"
    k = width_cap_step(oracle, q, d, 64, 400)
    assert k == 374 and len(widths(oracle.wfa(q, d, max_steps=k).stdout)) == 184
    texts, res = _paths(saln, [q], [d], 400)
    _check_expected(texts, res, [expected(oracle, q, d, 400, 64)], "pair 105")
    assert all(int(r["steps"][0]) == k for r in res.values())


# pairs by the number of expand calls after which the oracle converges
CONVERGING = {
    28: (b"CC", b"AGCTAC"), 30: (b"ACA", b"ACA"), 32: (b"AC", b"CAACAAG"),
    34: (b"ACGAAT", b"CAGAAT"), 36: (b"CACCCCAC", b"ACCCAAAAACA"),
    60: (b"CAGC", b"GCTTTGAACGCGT"), 62: (b"C", b"AACCCAACACC"), 64: (b"AG", b"TTTAAGTCTC"),
    66: (b"AACAC", b"CAAACCACACACC"), 68: (b"T", b"ACCGGAACTCTA"),
}
NEVER = [A21, (b"ACGT", b"ACGT"), (b"", b"ACG"), (b"", b""), (b"A", b"")]


def test_two_pass_boundary(saln, oracle):
    """Pairs that converge at, just below and just above 32 and 64 expand
    calls, and pairs that never converge, at step caps on both sides of both
    values and at 1, 2, 3 (the arena holds max_steps / 2 + 1 slots): all
    three paths equal one oracle run at the cap, whatever the first pass's
    own cap is.  The default width cannot bind at these caps (<= 127)."""
    for steps, (q, d) in CONVERGING.items():
        o = oracle.wfa(q, d, max_steps=200)
        assert (o.status, o.steps) == (oracle.WFA_OK, steps), (q, d)
    cases = list(CONVERGING.values()) + NEVER
    qs, ds = [c[0] for c in cases], [c[1] for c in cases]
    for cap in (1, 2, 3, 30, 31, 32, 33, 34, 35, 63, 64, 65, 66):
        exp = [oracle.wfa(q, d, max_steps=cap) for q, d in cases]
        texts, res = _paths(saln, qs, ds, cap)
        _check_expected(texts, res, exp, cap)
        conv = {s for s, e in zip(CONVERGING, exp) if e.status == oracle.WFA_OK}
        assert conv == {s for s in CONVERGING if s <= cap}, cap


def _lanes(budget_mb, max_steps, width, n):
    """Lanes per launch of a pass (include/saln.h, "wfa.arena_mb"), free
    memory permitting."""
    S = max_steps // 2 + 1
    per_lane = S * 48 + S * 3 * width * 8 + S
    return min(n, max(256, (budget_mb << 20) // per_lane))


def test_chunked_launches(saln, saln_opt, oracle):
    """600 pairs at a 1 MB arena budget: launches of 256 lanes, so the first
    pass takes three launches (the last one partial) and the re-run pass,
    fed from the re-run list in whatever order the first pass's lanes
    appended to it, at least two.  Results equal the oracle, the default
    budget's single launches and a second run; a plan executed twice reuses
    the re-run pass's larger arena for the next first pass."""
    cap, width = 200, 2 * (200 // 4) + 1  # a width that cannot bind at this cap
    long_, short = [], []
    for q, d in dict.fromkeys(seeded_pairs(41, 1500, max_len=20)):
        o = oracle.wfa(q, d, max_steps=cap)
        (long_ if o.steps > 64 else short).append((q, d, o))
    assert len(long_) >= 300 and len(short) >= 300
    cases = [c for ab in zip(long_[:300], short[:300]) for c in ab]
    qs, ds = [c[0] for c in cases], [c[1] for c in cases]
    n, n_rerun = len(cases), 300  # the pairs past 64 calls reach any first pass's cap
    pairs = [(k, k) for k in range(n)]
    kw = {"max_steps": cap, "max_width": width}
    ref, _ = saln.wfa_align_batch(qs, ds, pairs=pairs, **kw)
    assert _lanes(32768, cap, width, n) == n  # one launch per pass
    saln_opt("wfa.arena_mb", 1)
    assert _lanes(1, 64, width, n) == 256 < n  # whatever the first pass's cap up to 64
    assert _lanes(1, cap, width, n_rerun) == 256 < n_rerun
    texts, res = _paths(saln, qs, ds, cap, width)
    _check_expected(texts, res, [c[2] for c in cases], "1 MB")
    again, _ = saln.wfa_align_batch(qs, ds, pairs=pairs, **kw)
    twice = _plan_run(saln, qs, ds, pairs, kw, executes=2)
    for name, r in [("batch", res["batch"]), ("again", again), ("plan", res["plan"]),
                    ("execute 1", twice[0]), ("execute 2", twice[1])]:
        for f in FIELDS:
            assert np.array_equal(r[f], ref[f]), (name, f)


P = bytes([0x41, 0x80, 0xff, 0x00, 0x43, 0x47, 0x54, 0x4e, 0x61, 0x0c, 0x7f, 0x81, 0x2d, 0x41])
# bytes that differ at every position, some in the top or the bottom bit only
U = bytes([0x41, 0x00, 0x7f, 0x80, 0x54, 0xff, 0x01, 0x43, 0x47, 0x10, 0x61, 0x2d])
V = bytes([0xc1, 0x01, 0xff, 0x00, 0x55, 0x7f, 0x00, 0x47, 0x43, 0x90, 0x41, 0x0c])


def _word_pairs():
    out = []
    for n in range(len(P)):
        run = P[:n]
        out.append((b"A" + run + b"G", b"C" + run + b"T"))       # ends in a differing byte
        out.append((b"A" + run + b"G", b"C" + run + b"G"))       # the run reaches both ends
        out.append((b"A" + run + b"GT", b"C" + run))             # ... the db's end only
        out.append((b"A" + run, b"C" + run + b"\x00"))           # ... the query's end only
        out.append((b"A" + run + b"G" + run, b"C" + run + b"T"))  # |q| != |d|
    for j in range(8):  # first difference at byte j, every later byte differs too
        out.append((b"A" + P[:j] + U[j:], b"C" + P[:j] + V[j:]))
        out.append((b"A" + P[:j] + V[j:], b"C" + P[:j] + U[j:] + b"AC"))
    return out


def _placed(seqs, r):
    """CSR record list in which every sequence of seqs starts at an offset
    = r (mod 4): each is preceded by a filler record of 0 to 3 bytes.
    Returns (records, index of each sequence)."""
    recs, idx, off = [], [], 0
    for s in seqs:
        pad = (r - off) % 4
        recs.append(b"\xa5" * pad)
        off += pad
        idx.append(len(recs))
        recs.append(s)
        off += len(s)
    return recs, idx


def test_word_extension_edges(saln, oracle):
    """extend_m compares four bytes per step (two aligned dword loads and a
    byte funnel shift per sequence, the first set bit of the XOR): runs of 0
    to 13 equal bytes that end in a differing byte or at either sequence's
    end, the first difference at each byte of two words with all later bytes
    differing, bytes >= 0x80, 0x00 and other non-ACGT values, with the
    sequences at all 16 (q_off & 3, db_off & 3) placements and the device
    buffers at byte shifts 1, 2 and 3."""
    cases = _word_pairs()
    for n in range(len(P)):  # the base pairs converge at call 4 with offset n + 1
        o = oracle.wfa(*cases[5 * n], max_steps=64)
        assert (o.status, o.steps) == (oracle.WFA_OK, 4) and f"\toffset: {n + 1}\n" in o.stdout
    exp = [oracle.wfa(q, d, max_steps=64) for q, d in cases]
    assert {oracle.WFA_OK, oracle.WFA_NONCONVERGED} <= {e.status for e in exp}
    for rq in range(4):
        for rd in range(4):
            qs, qi = _placed([c[0] for c in cases], rq)
            ds, di = _placed([c[1] for c in cases], rd)
            q_off, d_off = saln.pack_csr(qs)[1], saln.pack_csr(ds)[1]
            assert all(int(q_off[i]) & 3 == rq for i in qi)
            assert all(int(d_off[i]) & 3 == rd for i in di)
            pairs = list(zip(qi, di))
            texts, res = _paths(saln, qs, ds, 64, pairs=pairs)
            if rq == rd == 0:
                for sh in ((1, 2), (2, 3), (3, 1)):
                    res[f"plan shifted {sh}"], = _plan_run(saln, qs, ds, pairs, {"max_steps": 64}, sh)
            _check_expected(texts, res, exp, (rq, rd))
            for path, r in res.items():
                for f in FIELDS:
                    assert np.array_equal(r[f], res["render"][f]), (rq, rd, path, f)
