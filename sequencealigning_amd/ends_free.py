"""Ends-free affine-gap alignment: local, semi-global and overlap — a
separately labelled engine, NOT reference parity.

The reference only declares these modes (``ScoreTensor::Local`` /
``::SemiGlobal`` carry empty comments, needleman_wunsch_affine.rs:238-239,
:331-332, and ``n_w_align`` answers "not implemented", :433-434; ``n_w_align``
here keeps doing that).  This module computes what they are meant to: Gotoh
affine-gap alignment with free ends on the GPU (ends_free_kernels.hip), with
the NW paths' scoring (``{match, mismatch, gap_open, gap_extend}``, default
``{5, -4, -8, -6}``; a gap of length L costs gap_open + L * gap_extend) and
CIGAR format ('=' / 'X' columns, 'I' a query base against '-', 'D' a '-'
against a db base; the db is the reference sequence).

* ``Mode.Local``: the best-scoring pair of substrings (Smith-Waterman).
* ``Mode.SemiGlobal``: the whole query against a free db substring.
* ``OVERLAP`` (4, this engine's own: ``records.Mode`` mirrors the reference's
  three names): overlap (dovetail) alignment, all four ends free and no floor.
  A suffix of one sequence against a prefix of the other, or one sequence
  inside the other; no overlap with a positive score gives the empty
  alignment (score 0, no words, coordinates 0).

The definitions (recurrences, tie rules, the walk's fixed choices) are in
include/saln.h and DESIGN.md; the checkers are tests/ends_free_model.py and
tests/overlap_model.py.

``ends_free_align_batch`` and its one-pair forms take a query of at most
1,024 columns and a db of at most 65,000 rows.  ``ends_free_align_long_batch``,
``local_align_long``, ``semi_global_align_long`` and ``overlap_align_long`` take pairs of any length
within the range guard ((n + m + 2) * max|parameter| < 2^30): a pair above the
limits runs the chunked fill (ends_free_long_kernels.hip), every other pair
the same fills as before, with the same records and words.  With
``replay=True`` they call ``saln_ends_free_replay_align_batch``: a pair above
the limits keeps boundary columns and checkpoint rows in place of its n x m
trace codes and its alignment is walked tile by tile
(ends_free_replay_kernels.hip; ``replay_bytes`` is what it holds against
``trace_budget``, option ``ends_free.tile_rows`` the tile's db rows).  Records
and words are the same.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .nw import CigarBatch, pack_csr
from .records import Mode

DEFAULT_SCORING = (5, -4, -8, -6)
TRACE_CAP = _lib.TRACE_CAP    # per-pair status: trace codes larger than the whole budget
MAX_QUERY = 1024              # longest query (columns); saln_ends_free_pair_geometry
OVERLAP = 4                   # SALN_MODE_OVERLAP: a mode value, not a records.Mode member


def _mode(mode) -> int:
    if isinstance(mode, Mode):
        return {Mode.Global: 0, Mode.Local: 1, Mode.SemiGlobal: 2}[mode]
    return int(mode)


def _pair_lists(pairs, n_q, n_db):
    if pairs is None:
        return None, None, n_q * n_db
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]), len(pairs)


def _align_batch(entry, queries, dbs, pairs, mode, scoring, trace_budget, cigar, device):
    """saln_ends_free_align_batch or saln_ends_free_long_align_batch (entry)."""
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    pq, pd, n = _pair_lists(pairs, len(qo) - 1, len(do) - 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(getattr(L, entry)(
        _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq),
        vp(pd), n, _mode(mode), _lib.scoring_arg(scoring), int(trace_budget), int(bool(cigar)),
        C.byref(h)), entry)
    try:
        res = np.zeros(n, dtype=_lib.ENDS_FREE_RESULT_DTYPE)
        r = _lib.EndsFreeResult()
        for k in range(n):
            _lib.check(L.saln_ends_free_aln_get(h, k, C.byref(r), None), "saln_ends_free_aln_get")
            res[k] = (r.score, r.status, r.q_begin, r.q_end, r.db_begin, r.db_end, r.cigar_len,
                      r.reserved)
        total = int(res["cigar_len"].sum(dtype=np.uint64))
        words = np.zeros(total, np.uint32)
        if total:  # the handle's words are contiguous in pair order
            cp = C.POINTER(C.c_uint32)()
            _lib.check(L.saln_ends_free_aln_get(h, 0, None, C.byref(cp)), "saln_ends_free_aln_get")
            C.memmove(words.ctypes.data, cp, 4 * total)
    finally:
        L.saln_ends_free_aln_free(h)
    lens = res["cigar_len"].astype(np.uint64)
    offs = np.zeros(n, np.uint64)
    if n:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return res, CigarBatch(words, offs, lens)


def ends_free_align_batch(queries, dbs, pairs=None, *, mode, scoring=None, trace_budget: int = 0,
                          cigar: bool = True, device: int = 0):
    """Local, semi-global or overlap (mode=OVERLAP) alignment of a batch.
    pairs: None (all-vs-all, db
    outer / query inner) or (n, 2) (query index, db index).  Returns (results,
    cigars): results is a structured array (score, status, q_begin, q_end,
    db_begin, db_end, cigar_len; the ranges half-open and 0-based), cigars a
    CigarBatch (pair k's [(length, op), ...]).  cigar=False runs the fill only:
    score and ends, begins -1, no words.  A pair whose trace codes alone exceed
    trace_budget bytes (0 selects 1 GiB per chunk) has status TRACE_CAP, its
    score and ends, begins -1 and no words."""
    return _align_batch("saln_ends_free_align_batch", queries, dbs, pairs, mode, scoring,
                        trace_budget, cigar, device)


def ends_free_align_long_batch(queries, dbs, pairs=None, *, mode, scoring=None,
                               trace_budget: int = 0, cigar: bool = True, device: int = 0,
                               replay: bool = False):
    """ends_free_align_batch without the length limits
    (saln_ends_free_long_align_batch): the same arguments and return.  A pair
    of at most 1,024 x 65,000 runs as there and gives the same record and
    words; every other pair runs the chunked fill.  The only limit is the
    range guard.  replay=True (saln_ends_free_replay_align_batch): the same
    records and words, but a pair of the chunked fill holds replay_bytes, not
    trace_bytes_long, against trace_budget, and its alignment comes from the
    tiled replay; TRACE_CAP then means that replay_bytes alone exceed the
    budget."""
    entry = "saln_ends_free_replay_align_batch" if replay else "saln_ends_free_long_align_batch"
    return _align_batch(entry, queries, dbs, pairs, mode, scoring, trace_budget, cigar, device)


def _one(seq1, seq2, mode, scoring, trace_budget, device, batch=ends_free_align_batch, **kw):
    res, cig = batch([seq1], [seq2], [(0, 0)], mode=mode, scoring=scoring,
                     trace_budget=trace_budget, device=device, **kw)
    return res[0], cig[0]


def local_align(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0):
    """(result record, cigar) of the best local alignment of seq1 (query)
    and seq2 (db): seq1[q_begin:q_end] against seq2[db_begin:db_end]."""
    return _one(seq1, seq2, Mode.Local, scoring, trace_budget, device)


def semi_global_align(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0):
    """(result record, cigar) of the whole of seq1 (query) against the best
    window seq2[db_begin:db_end] of the db."""
    return _one(seq1, seq2, Mode.SemiGlobal, scoring, trace_budget, device)


def overlap_align(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0):
    """(result record, cigar) of the best overlap (dovetail) alignment of seq1
    (query) and seq2 (db): seq1[q_begin:q_end] against seq2[db_begin:db_end],
    each range touching an end of its sequence; score 0 and no words when no
    overlap scores above 0."""
    return _one(seq1, seq2, OVERLAP, scoring, trace_budget, device)


def local_align_long(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0,
                     replay: bool = False):
    """local_align for sequences of any length (ends_free_align_long_batch)."""
    return _one(seq1, seq2, Mode.Local, scoring, trace_budget, device, ends_free_align_long_batch,
                replay=replay)


def semi_global_align_long(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0,
                           replay: bool = False):
    """semi_global_align for sequences of any length (ends_free_align_long_batch)."""
    return _one(seq1, seq2, Mode.SemiGlobal, scoring, trace_budget, device,
                ends_free_align_long_batch, replay=replay)


def overlap_align_long(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0,
                       replay: bool = False):
    """overlap_align for sequences of any length (ends_free_align_long_batch)."""
    return _one(seq1, seq2, OVERLAP, scoring, trace_budget, device, ends_free_align_long_batch,
                replay=replay)


def cigar_score(cigar, scoring=None) -> int:
    """Affine-gap score of a CIGAR ([(n, op)]): match per '=' column, mismatch
    per 'X' column, gap_open + gap_extend * len per gap run ('I' or 'D')."""
    m, x, o, e = scoring if scoring is not None else DEFAULT_SCORING
    total, prev = 0, None
    for n, op in cigar:
        if op == "=":
            total += m * n
        elif op == "X":
            total += x * n
        else:
            total += e * n + (o if op != prev else 0)
        prev = op
    return total


def trace_bytes(len_q: int, len_db: int) -> int:
    """saln_ends_free_trace_bytes: bytes of trace codes of one pair (host only)."""
    out = C.c_uint64()
    _lib.check(_lib.lib().saln_ends_free_trace_bytes(int(len_q), int(len_db), C.byref(out)),
               "saln_ends_free_trace_bytes")
    return out.value


def trace_bytes_long(len_q: int, len_db: int) -> int:
    """saln_ends_free_long_trace_bytes: bytes of trace codes of one pair under
    ends_free_align_long_batch (host only); trace_bytes within its limits."""
    out = C.c_uint64()
    _lib.check(_lib.lib().saln_ends_free_long_trace_bytes(int(len_q), int(len_db), C.byref(out)),
               "saln_ends_free_long_trace_bytes")
    return out.value


def replay_bytes(len_q: int, len_db: int, tile_rows: int = 0) -> int:
    """saln_ends_free_replay_bytes: bytes one pair holds against trace_budget
    under replay=True (host only).  trace_bytes within the class limits; above
    them the boundary columns, the checkpoint rows and one tile of codes.
    tile_rows 0: the value of option ends_free.tile_rows."""
    out = C.c_uint64()
    _lib.check(_lib.lib().saln_ends_free_replay_bytes(int(len_q), int(len_db), int(tile_rows),
                                                      C.byref(out)),
               "saln_ends_free_replay_bytes")
    return out.value


def pair_path_long(len_q: int, len_db: int) -> tuple[int, int]:
    """saln_ends_free_long_pair_path: (long_fill, chunks) of one pair under
    ends_free_align_long_batch (host only): 1 and its 1,024-column chunks when
    it runs the chunked fill, (0, 1) when it runs a class fill."""
    lf, chunks = C.c_int32(), C.c_uint32()
    _lib.check(_lib.lib().saln_ends_free_long_pair_path(int(len_q), int(len_db), C.byref(lf),
                                                        C.byref(chunks)),
               "saln_ends_free_long_pair_path")
    return lf.value, chunks.value


def pair_geometry(len_q: int) -> tuple[int, int]:
    """saln_ends_free_pair_geometry: (lanes, columns per lane) of the class a
    query of len_q columns runs in (host only).  Raises SalnError (E_INVALID)
    above MAX_QUERY."""
    lanes, cols = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().saln_ends_free_pair_geometry(int(len_q), C.byref(lanes), C.byref(cols)),
               "saln_ends_free_pair_geometry")
    return lanes.value, cols.value


class EndsFreePlan:
    """Device-resident score-only batch: plan from host offsets and a pair
    list once, execute on device (torch) sequence buffers into a device tensor
    of result records (n_pairs x 8 int32: score, status, q_begin = -1, q_end,
    db_begin = -1, db_end, 0, 0)."""

    def __init__(self, q_off, db_off, pairs=None, *, mode, scoring=None, device: int = 0):
        L = _lib.lib()
        self._L = L
        self.device = device
        qo = np.ascontiguousarray(q_off, np.uint64)
        do = np.ascontiguousarray(db_off, np.uint64)
        pq, pd, n = _pair_lists(pairs, len(qo) - 1, len(do) - 1)
        self.n_pairs = n
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._h = C.c_void_p()
        _lib.check(L.saln_ends_free_plan_create(_lib.context(device), vp(qo), len(qo) - 1, vp(do),
                                                len(do) - 1, vp(pq), vp(pd), n, _mode(mode),
                                                _lib.scoring_arg(scoring), C.byref(self._h)),
                   "saln_ends_free_plan_create")

    def execute(self, d_q, d_db, d_results, stream=None):
        """d_q / d_db: device uint8 tensors (CSR bytes), d_results: device
        int32[n_pairs * 8] (view it with _lib.ENDS_FREE_RESULT_DTYPE on the host)."""
        assert d_results.numel() * d_results.dtype.itemsize >= 32 * self.n_pairs
        if stream is None:  # torch's current stream, like NwPlan.execute
            stream = _lib.torch_stream(d_results.device)
        _lib.check(self._L.saln_ends_free_execute(
            self._h, C.c_void_p(d_q.data_ptr()), C.c_void_p(d_db.data_ptr()),
            C.c_void_p(d_results.data_ptr()), C.c_void_p(stream)), "saln_ends_free_execute")

    def close(self):
        if self._h:
            self._L.saln_ends_free_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
