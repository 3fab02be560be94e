"""Corrected gap-affine WFA — a separately labelled
engine, NOT reference parity.

The reference's ``wfa_align`` (src/wfa.rs:23-42; ``sequencealigning_amd.wfa``
reproduces it exactly) defines no output for realistic inputs: Ocean::trim
panics at s = 20.  This module computes what a gap-affine
WFA is meant to compute with the reference's penalties (wfa.rs:14-21,
x = 4 mismatch, o = 2 gap open, e = 6 gap extend; a gap of length L costs
o + L*e): the minimum penalty of a global alignment, on the GPU
(wfa_affine_kernels.hip).  The checker is the Gotoh DP in
``oracle/refaffine.c``.

``wfa_affine_align_batch`` / ``wfa_affine_align`` also return one optimal
alignment per pair as a CIGAR in the NW paths' format
(wfa_affine_trace_kernels.hip): '=' / 'X' columns, 'I' a query base against
'-', 'D' a '-' against a db base (the db is the reference sequence).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .nw import CigarBatch, _decode_cigar, pack_csr

DEFAULT_PENALTIES = (4, 2, 6)
OVER_MAX_SCORE = -1   # penalty above max_score
OVER_WIDTH = -2       # wavefront wider than the second pass's ring: 2,048 diagonals with
#                       the default penalties, fewer where the penalties need more ring
#                       slots or a sequence is above 32,000 bases (plan_geometry reports it)
TRACE_CAP = _lib.TRACE_CAP    # per-pair status: trace codes larger than the whole budget
INTERNAL = _lib.INTERNAL      # per-pair status: trace / score passes disagree (never expected)


def _pen(penalties):
    x, o, e = penalties if penalties is not None else DEFAULT_PENALTIES
    return _lib.WfaPenalties(int(x), int(o), int(e))


def wfa_affine_batch(queries, dbs, pairs=None, *, penalties=None, max_score: int = 0,
                     device: int = 0) -> np.ndarray:
    """Minimum gap-affine penalty per pair (int32; negative codes above).
    pairs: None (all-vs-all, db outer / query inner like main.rs:61-62) or
    (n, 2) (query index, db index)."""
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    if pairs is None:
        n = (len(qo) - 1) * (len(do) - 1)
        pq = pd = None
    else:
        pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
        n = len(pairs)
        pq = np.ascontiguousarray(pairs[:, 0])
        pd = np.ascontiguousarray(pairs[:, 1])
    out = np.zeros(n, np.int32)
    if n == 0:
        return out
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    pen = _pen(penalties)
    _lib.check(_lib.lib().saln_wfa_affine_batch(
        _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq),
        vp(pd), n, C.byref(pen), int(max_score), vp(out)), "saln_wfa_affine_batch")
    return out


def wfa_affine(seq1: bytes, seq2: bytes, *, penalties=None, max_score: int = 0,
               device: int = 0) -> int:
    """Minimum gap-affine penalty of one pair (seq1 = query, seq2 = db)."""
    return int(wfa_affine_batch([seq1], [seq2], [(0, 0)], penalties=penalties,
                                max_score=max_score, device=device)[0])


def _pair_args(queries, dbs, pairs):
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    if pairs is None:
        n = (len(qo) - 1) * (len(do) - 1)
        pq = pd = None
    else:
        pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
        n = len(pairs)
        pq = np.ascontiguousarray(pairs[:, 0])
        pd = np.ascontiguousarray(pairs[:, 1])
    return qs, qo, ds, do, pq, pd, n


def wfa_affine_align_batch(queries, dbs, pairs=None, *, penalties=None, max_score: int = 0,
                           trace_budget: int = 0, device: int = 0):
    """Minimum gap-affine penalty and one optimal alignment per pair.
    Returns (results, cigars): results is a structured array (score, status,
    cigar_len; score as wfa_affine_batch), cigars a CigarBatch (pair k's
    [(length, op), ...], empty where the pair has no alignment: a negative
    score, or status TRACE_CAP when its trace codes alone exceed
    trace_budget bytes; 0 selects 1 GiB per chunk).  pairs as wfa_affine_batch."""
    qs, qo, ds, do, pq, pd, n = _pair_args(queries, dbs, pairs)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    L = _lib.lib()
    pen = _pen(penalties)
    h = C.c_void_p()
    _lib.check(L.saln_wfa_affine_align_batch(
        _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq),
        vp(pd), n, C.byref(pen), int(max_score), int(trace_budget), C.byref(h)),
        "saln_wfa_affine_align_batch")
    try:
        res = np.zeros(n, dtype=_lib.WFA_AFFINE_RESULT_DTYPE)
        r = _lib.WfaAffineResult()
        for k in range(n):
            _lib.check(L.saln_wfa_affine_aln_get(h, k, C.byref(r), None),
                       "saln_wfa_affine_aln_get")
            res[k] = (r.score, r.status, r.cigar_len, 0)
        total = int(res["cigar_len"].sum(dtype=np.uint64))
        words = np.zeros(total, np.uint32)
        if total:  # the handle's words are contiguous in pair order
            cp = C.POINTER(C.c_uint32)()
            _lib.check(L.saln_wfa_affine_aln_get(h, 0, None, C.byref(cp)),
                       "saln_wfa_affine_aln_get")
            C.memmove(words.ctypes.data, cp, 4 * total)
    finally:
        L.saln_wfa_affine_aln_free(h)
    lens = res["cigar_len"].astype(np.uint64)
    offs = np.zeros(n, np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return res, CigarBatch(words, offs, lens)


def wfa_affine_align(seq1: bytes, seq2: bytes, *, penalties=None, max_score: int = 0,
                     trace_budget: int = 0, device: int = 0):
    """(score, cigar) of one pair (seq1 = query, seq2 = db): cigar is the NW
    path's [(n, op)] list (nw.alignment_rows prints it), empty without an
    alignment (negative score, or a trace larger than trace_budget)."""
    res, cig = wfa_affine_align_batch([seq1], [seq2], [(0, 0)], penalties=penalties,
                                      max_score=max_score, trace_budget=trace_budget,
                                      device=device)
    return int(res["score"][0]), cig[0]


def cigar_penalty(cigar, penalties=None) -> int:
    """Gap-affine penalty of a CIGAR ([(n, op)]): x per 'X' column and
    o + e * len per gap run ('I' or 'D'; an I run next to a D run is two gaps)."""
    x, o, e = penalties if penalties is not None else DEFAULT_PENALTIES
    total, prev = 0, None
    for n, op in cigar:
        if op == "X":
            total += x * n
        elif op in "ID":
            total += e * n + (o if op != prev else 0)
        prev = op
    return total


def trace_bytes(len_q: int, len_db: int, score: int, penalties=None) -> int:
    """saln_wfa_affine_trace_bytes: bytes of trace workspace of one pair with
    this penalty (host only; the layout is in DESIGN.md)."""
    pen = _pen(penalties)
    out = C.c_uint64()
    _lib.check(_lib.lib().saln_wfa_affine_trace_bytes(C.byref(pen), int(len_q), int(len_db),
                                                      int(score), C.byref(out)),
               "saln_wfa_affine_trace_bytes")
    return out.value


def plan_geometry(lengths, penalties=None):
    """saln_wfa_affine_plan_geometry (host only): the two passes a plan over
    pairs of these (len_q, len_db) takes with the process's options, as a
    list of two dicts (ring_width, seqcap, lds_bytes, i32_offsets,
    workgroups_per_cu).  Raises
    SalnError (E_INVALID) where the plan would be refused."""
    lens = np.asarray(list(lengths), np.uint64).reshape(-1, 2)
    lq = np.ascontiguousarray(lens[:, 0])
    ld = np.ascontiguousarray(lens[:, 1])
    pen = _pen(penalties)
    out = (_lib.WfaAffinePassGeometry * 2)()
    _lib.check(_lib.lib().saln_wfa_affine_plan_geometry(
        C.byref(pen), lq.ctypes.data_as(C.c_void_p), ld.ctypes.data_as(C.c_void_p), len(lens),
        out), "saln_wfa_affine_plan_geometry")
    return [dict(ring_width=g.ring_width, seqcap=g.seqcap, lds_bytes=g.lds_bytes,
                 i32_offsets=bool(g.i32_offsets), workgroups_per_cu=g.workgroups_per_cu)
            for g in out]


class WfaAffinePlan:
    """Device-resident corrected-WFA batch: plan from host offsets and a pair
    list once, execute on device (torch) sequence buffers into a device int32
    score tensor."""

    def __init__(self, q_off, db_off, pairs=None, *, penalties=None, max_score: int = 0,
                 device: int = 0):
        L = _lib.lib()
        self._L = L
        qo = np.ascontiguousarray(q_off, np.uint64)
        do = np.ascontiguousarray(db_off, np.uint64)
        if pairs is None:
            n = (len(qo) - 1) * (len(do) - 1)
            pq = pd = None
        else:
            pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
            n = len(pairs)
            pq = np.ascontiguousarray(pairs[:, 0])
            pd = np.ascontiguousarray(pairs[:, 1])
        self.n_pairs = n
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._h = C.c_void_p()
        pen = _pen(penalties)
        _lib.check(L.saln_wfa_affine_plan_create(_lib.context(device), vp(qo), len(qo) - 1,
                                                 vp(do), len(do) - 1, vp(pq), vp(pd), n,
                                                 C.byref(pen), int(max_score), C.byref(self._h)),
                   "saln_wfa_affine_plan_create")

    def execute(self, d_q, d_db, d_scores, stream=None):
        """d_q / d_db: device uint8 tensors (CSR bytes), d_scores: device int32[n_pairs]."""
        assert d_scores.numel() >= self.n_pairs and d_scores.dtype.itemsize == 4
        if stream is None:  # torch's current stream, like NwPlan.execute
            stream = _lib.torch_stream(d_scores.device)
        _lib.check(self._L.saln_wfa_affine_execute(
            self._h, C.c_void_p(d_q.data_ptr()), C.c_void_p(d_db.data_ptr()),
            C.c_void_p(d_scores.data_ptr()), C.c_void_p(stream)), "saln_wfa_affine_execute")

    def close(self):
        if self._h:
            self._L.saln_wfa_affine_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
