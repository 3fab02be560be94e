"""Shared helpers of the corrected gap-affine WFA tests: a plain model of the
engine and the CIGAR checker (test-only).

The model is a dictionary-based gap-affine WFA in Python integers, written
from the header comments of wfa_affine_kernels.hip (recurrences, ranges) and
wfa_affine_trace_kernels.hip (origin codes, tie-break, orientation).  It
shares no code with the engine.

Wavefronts (query v, db h, diagonal k = h - v, an entry is the furthest h):
    I[t][k] = max(M[t - toe][k-1], I[t - te][k-1]) + 1
    D[t][k] = max(M[t - toe][k+1], D[t - te][k+1])
    M[t][k] = max(M[t - tx][k] + 1, I[t][k], D[t][k]), then extended
in steps of g = gcd(x, o+e, e) (tx = x/g, toe = (o+e)/g, te = e/g).  The
first t with M[t][ld - lq] == ld gives the penalty t * g.

Ranges: the engine keeps a diagonal range per component and step, computed
from the sources' ranges alone (clamped to [-lq, ld]), so they depend only on
the lengths and the penalties; a step whose M range is wider than the ring
ends the pass (checked before the step's convergence test).

Tie-break: M prefers X (the mismatch), then I, then D; a gap prefers extend
over open.  Orientation: the I component advances the db - CIGAR 'D'; the D
component advances the query - CIGAR 'I'.
"""
from __future__ import annotations

from math import gcd

import numpy as np


def check_cigar(saln, q, d, cigar, score, pen, want=None):
    """The shared checker; want: the DP's penalty (None: not compared)."""
    for (n, op), nxt in zip(cigar, cigar[1:] + [(1, None)]):
        assert n > 0 and op in "=XID" and op != nxt[1], cigar
    i = j = 0  # db, query
    for n, op in cigar:
        if op in "=X":
            a = np.frombuffer(q, np.uint8, n, j)
            b = np.frombuffer(d, np.uint8, n, i)
            assert ((a == b) if op == "=" else (a != b)).all(), (op, i, j)
            i += n
            j += n
        elif op == "I":
            j += n
        else:
            i += n
        assert j <= len(q) and i <= len(d)
    assert (j, i) == (len(q), len(d))
    assert saln.wfa_affine.cigar_penalty(cigar, pen) == score
    if want is not None:
        assert score == want


def mixed_pairs(seed, n=96, max_len=400):
    """The recipe of test_wfa_affine_gpu.py::_pairs with n pairs of at most
    about max_len bases (the lopsided db: 1.25 max_len), plus the four pairs
    with an empty side / identical."""
    from sequencealigning_amd import synth
    rng = np.random.default_rng(seed)
    qs, ds = [], []
    for k in range(n):
        kind = k % 6
        lq = int(rng.integers(1, max_len))
        if kind == 0:   # i.i.d.
            q = synth.random_bases(seed * 1000 + k, lq).tobytes()
            d = synth.random_bases(seed * 1000 + k + 500, int(rng.integers(1, max_len))).tobytes()
        elif kind == 1:  # mutated 5 %
            q = synth.random_bases(seed * 1000 + k, lq).tobytes()
            d = synth.mutate(q, 0.05, seed=k)
        elif kind == 2:  # mutated 20 %
            q = synth.random_bases(seed * 1000 + k, lq).tobytes()
            d = synth.mutate(q, 0.2, seed=k)
        elif kind == 3:  # repetitive, 2 letters
            q = bytes(rng.choice([65, 67], lq).astype(np.uint8))
            d = bytes(rng.choice([65, 67], int(rng.integers(1, max_len))).astype(np.uint8))
        elif kind == 4:  # identical / prefix
            q = synth.random_bases(seed * 1000 + k, lq).tobytes()
            d = q[: int(rng.integers(0, lq + 1))]
        else:           # lopsided, with N
            q = bytes(rng.choice(list(b"ACGTN"), int(rng.integers(1, 30))).astype(np.uint8))
            d = bytes(rng.choice(list(b"ACGTN"),
                                 int(rng.integers(max_len // 4, max_len + max_len // 4))
                                 ).astype(np.uint8))
        qs.append(q)
        ds.append(d)
    qs += [b"", b"A", b"", b"ACGT"]
    ds += [b"", b"", b"ACG", b"ACGT"]
    return qs, ds


# ------------------------------------------------------------------ ranges
def _units(pen):
    x, o, e = pen
    g = gcd(gcd(x, o + e), e)
    return g, x // g, (o + e) // g, e // g


class Ranges:
    """The engine's per-step diagonal ranges of one pair shape: step(t) ->
    (M, I, D) ranges, each (lo, hi) or None; steps are computed in order."""

    def __init__(self, lq, ld, pen):
        self.lq, self.ld = lq, ld
        self.g, self.tx, self.toe, self.te = _units(pen)
        self.m = {0: (0, 0)}
        self.i = {0: None}
        self.d = {0: None}
        self.done = 0

    def _clamp(self, lo, hi):
        lo, hi = max(lo, -self.lq), min(hi, self.ld)
        return (lo, hi) if lo <= hi else None

    @staticmethod
    def _hull(*rs):
        rs = [r for r in rs if r is not None]
        return (min(r[0] for r in rs), max(r[1] for r in rs)) if rs else None

    def step(self, t):
        while self.done < t:
            s = self.done + 1
            mo, mx = self.m.get(s - self.toe), self.m.get(s - self.tx)
            ie, de = self.i.get(s - self.te), self.d.get(s - self.te)
            hi_ = self._hull(mo, ie)
            hd_ = self._hull(mo, de)
            ir = self._clamp(hi_[0] + 1, hi_[1] + 1) if hi_ else None
            dr = self._clamp(hd_[0] - 1, hd_[1] - 1) if hd_ else None
            xr = self._clamp(*mx) if mx else None
            self.m[s], self.i[s], self.d[s] = self._hull(ir, dr, xr), ir, dr
            # the rings keep only the last max(tx, toe) / te steps
            self.m.pop(s - max(self.tx, self.toe) - 1, None)
            self.i.pop(s - self.te - 1, None)
            self.d.pop(s - self.te - 1, None)
            self.done = s
        return self.m[t], self.i[t], self.d[t]


_shapes = {}  # (lq, ld, pen) -> (Ranges, widths so far): they depend on nothing else


def m_widths(lq, ld, pen, penalty):
    """mHi - mLo + 1 of steps 1 .. penalty / g (0 for a step with no cell)."""
    g = _units(pen)[0]
    assert penalty % g == 0
    r, out = _shapes.setdefault((lq, ld, tuple(pen)), (Ranges(lq, ld, pen), []))
    for t in range(len(out) + 1, penalty // g + 1):
        m = r.step(t)[0]
        out.append(m[1] - m[0] + 1 if m else 0)
    return out[:penalty // g]


def verdict(lq, ld, pen, penalty, w1, w2):
    """Where a pair with this (true) penalty gets its score: 1 (first pass,
    ring w1), 2 (second pass, ring w2) or -2 (wider than both)."""
    if lq == 0 or ld == 0:
        return 1
    widest = max(m_widths(lq, ld, pen, penalty), default=1)
    return 1 if widest <= w1 else 2 if widest <= w2 else -2


# ------------------------------------------------------------------- model
def _extend(q, d, v, h):
    while v < len(q) and h < len(d) and q[v] == d[h]:
        v += 1
        h += 1
    return h


def _ge(a, b):
    """a >= b with None as -inf (both -inf: equal)."""
    return b is None or (a is not None and a >= b)


def _mx(a, b):
    return b if a is None else a if b is None else max(a, b)


def wfa_align(q: bytes, d: bytes, pen, max_steps=1 << 20):
    """(penalty, M-range widths of steps 1 .. T, CIGAR [(n, op)]) of one pair
    under the documented tie-break."""
    x, o, e = pen
    lq, ld = len(q), len(d)
    if lq == 0 or ld == 0:
        cig = ([(lq, "I")] if lq else []) + ([(ld, "D")] if ld else [])
        return (o + e * (lq + ld) if lq + ld else 0), [], cig
    g, tx, toe, te = _units(pen)
    kend = ld - lq
    rng = Ranges(lq, ld, pen)
    h0 = _extend(q, d, 0, 0)
    # per step: M (extended), I, D offsets and the trace records
    M, I, D = {0: {0: h0}}, {0: {}}, {0: {}}
    pre = {0: {0: 0}}      # pre-extension M
    msrc = {0: {}}         # 'X' | 'I' | 'D'
    iext, dext = {0: {}}, {0: {}}
    widths = []
    T = 0
    if not (kend == 0 and h0 >= ld):
        for t in range(1, max_steps + 1):
            mr, _, _ = rng.step(t)
            M[t], I[t], D[t], pre[t], msrc[t], iext[t], dext[t] = {}, {}, {}, {}, {}, {}, {}
            widths.append(mr[1] - mr[0] + 1 if mr else 0)
            if mr is None:
                continue
            Mo, Mx = M.get(t - toe, {}), M.get(t - tx, {})
            Ie, De = I.get(t - te, {}), D.get(t - te, {})

            def cell(h, k):
                return h is not None and 0 <= h <= ld and h - k <= lq

            for k in range(mr[0], mr[1] + 1):
                mo_l, ie = Mo.get(k - 1), Ie.get(k - 1)
                mo_r, de = Mo.get(k + 1), De.get(k + 1)
                i_ = _mx(mo_l, ie)
                i_ = i_ + 1 if i_ is not None else None
                i_ = i_ if cell(i_, k) else None
                d_ = _mx(mo_r, de)
                d_ = d_ if cell(d_, k) else None
                x_ = Mx.get(k)
                x_ = x_ + 1 if x_ is not None else None
                x_ = x_ if cell(x_, k) else None
                if i_ is not None:
                    I[t][k] = i_
                    iext[t][k] = _ge(ie, mo_l)
                if d_ is not None:
                    D[t][k] = d_
                    dext[t][k] = _ge(de, mo_r)
                m_ = _mx(x_, _mx(i_, d_))
                if m_ is None:
                    continue
                assert m_ - k >= 0
                msrc[t][k] = "X" if _ge(x_, _mx(i_, d_)) else "I" if _ge(i_, d_) else "D"
                pre[t][k] = m_
                M[t][k] = _extend(q, d, m_ - k, m_)
            if M[t].get(kend, -1) >= ld:
                T = t
                break
        else:
            raise AssertionError("no convergence")
    # walk back from (T, kend, M); ops collected in reverse
    ops = []
    t, k, comp = T, kend, "M"
    while True:
        if comp == "M":
            ops.append(("=", M[t][k] - pre[t][k]))
            if t == 0:
                assert k == 0
                break
            s = msrc[t][k]
            if s == "X":
                ops.append(("X", 1))
                t -= tx
            else:
                comp = s
        elif comp == "I":   # a '-' against a db base
            ops.append(("D", 1))
            ext = iext[t][k]
            k -= 1
            t -= te if ext else toe
            comp = "I" if ext else "M"
        else:               # a query base against '-'
            ops.append(("I", 1))
            ext = dext[t][k]
            k += 1
            t -= te if ext else toe
            comp = "D" if ext else "M"
    cig = []
    for op, n in reversed(ops):
        if n == 0:
            continue
        if cig and cig[-1][1] == op:
            cig[-1] = (cig[-1][0] + n, op)
        else:
            cig.append((n, op))
    return T * g, widths, cig
