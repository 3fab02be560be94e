"""Ends-free affine-gap alignment: local, semi-global, overlap and extension —
a separately labelled engine, NOT reference parity.

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
* ``EXTEND`` (8, this engine's own as well): extension alignment, the gapped
  extension step of seed-and-extend.  The alignment is pinned at the origin
  (both sequences' first bytes, the anchor) and free at its end: it may stop
  at any cell, with no charge for what lies behind the stop.  Column 0 is a
  deletion run and row 0 an insertion run, so an alignment may begin with
  either.  No prefix pair with a positive score gives the empty alignment
  (score 0, no words, coordinates 0).  ``extend_align(..., direction="left")``
  extends leftwards from an anchor at the sequences' ends.

``xdrop=X`` (an int >= 0; ``ends_free_align_batch``, ``extend_align`` and
``EndsFreePlan``, mode EXTEND only) is the X-drop extension
(``saln_ends_free_xdrop_*``): a cell whose value lies more than X below the
best unpruned value above and left of it is pruned, so the alignment cannot
cross a stretch that costs more than X, and the fill leaves a pair once
nothing unpruned is left on its front.  The result depends only on the pair,
the scoring and X; a very large X gives plain extension's.  The records'
``reserved`` then holds the fill's row-loop steps (``xdrop_steps``).  The
``*_long`` functions take no ``xdrop``; X-drop extension of pairs of any
length is ``xdrop_extend_long_batch`` / ``xdrop_extend_long``
(``saln_ends_free_xdrop_long_*``): a pair above the limits runs the chunked
X-drop fill (ends_free_xdrop_long_kernels.hip), which runs a chunk of 1,024
query columns only over the rows between its first and last unpruned cell and
leaves the pair at the first chunk without one.  With ``replay=True`` they
call ``saln_ends_free_xdrop_replay_align_batch``: such a pair keeps, for the
rows each chunk ran, boundary columns and checkpoint rows (with B) in place of
its codes, and its words come from the tiled replay
(ends_free_xdrop_replay_kernels.hip; ``xdrop_replay_bytes``).

The definitions (recurrences, tie rules, the walk's fixed choices) are in
include/saln.h and DESIGN.md; the checker of the four modes under both kinds
of scoring is tests/ends_free_model.py.

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

``score_batch`` and ``EndsFreeScorePlan`` (``saln_ends_free_score_*``) answer a
search's first question, what each pair scores, and nothing else: one int32 per
pair, exactly ``ends_free_align_batch``'s ``score``, in all four modes.  Local
and semi-global pairs whose values fit 16 bits (``score_path``) run the
packed-i16 fill (ends_free_score_kernels.hip), two pairs to a lane group; every
other pair runs the i32 fill.  Same length limits as ``ends_free_align_batch``.

Every ``scoring=`` argument takes the 4-tuple above or a ``SubstitutionMatrix``
(protein scoring under a BLOSUM or PAM style table, IUPAC codes, transition /
transversion scoring): s(i, j) = scores[symbol of the db byte][symbol of the
query byte], everything else as defined above; '=' and 'X' stay byte
comparisons.  A matrix runs the ``saln_ends_free_sub_*`` entry points, a
4-tuple exactly the ones it always ran.
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
EXTEND = 8                    # SALN_MODE_EXTEND: likewise


class SubstitutionMatrix:
    """A substitution matrix with its gap costs: scoring of the ends-free
    functions in place of the (match, mismatch, gap_open, gap_extend) tuple.

    alphabet: the symbols, one byte each, at most 31.  scores[a][b]: the db
    symbol alphabet[a] against the query symbol alphabet[b], each within int8;
    the table need not be symmetric.  A byte outside the alphabet maps to one
    more symbol, which scores ``unknown`` against everything and everything
    against it (default: the smallest entry).  case_insensitive: a letter of
    the alphabet also stands for its other case.  Raises ValueError on a
    duplicate symbol, an entry outside int8, a table that is not
    len(alphabet) x len(alphabet), or more symbols than fit.

    The engine's domain (gap_open <= 0, gap_extend < 0, some entry > 0) is
    checked by the library when the matrix is used (SalnError, E_INVALID), and
    by ``check()``."""

    MAX_SYMBOLS = 31  # the 32nd is the unknown symbol

    def __init__(self, alphabet: bytes, scores, gap_open: int, gap_extend: int, *, unknown=None,
                 case_insensitive: bool = False):
        alphabet = bytes(alphabet)
        n = len(alphabet)
        if n == 0:
            raise ValueError("SubstitutionMatrix: the alphabet is empty")
        if n > self.MAX_SYMBOLS:
            raise ValueError(f"SubstitutionMatrix: {n} symbols, at most {self.MAX_SYMBOLS} fit "
                             "(one more is the unknown symbol)")
        rows = [list(r) for r in scores]
        if len(rows) != n or any(len(r) != n for r in rows):
            raise ValueError(f"SubstitutionMatrix: scores must be {n} x {n}, one row and one column "
                             "per symbol of the alphabet")
        table = [[int(v) for v in r] for r in rows]
        if any(int(v) != v for r in rows for v in r):
            raise ValueError("SubstitutionMatrix: entries must be integers")
        flat = [v for r in table for v in r]
        if unknown is None:
            unknown = min(flat)
        unknown = int(unknown)
        for v in flat + [unknown]:
            if not -128 <= v <= 127:
                raise ValueError(f"SubstitutionMatrix: entry {v} is outside int8")
        code = [n] * 256
        seen = set()
        for a, byte in enumerate(alphabet):
            keys = {byte}
            if case_insensitive:
                keys |= {ord(chr(byte).lower()), ord(chr(byte).upper())} if byte < 128 else set()
            if keys & seen:
                raise ValueError(f"SubstitutionMatrix: duplicate symbol {bytes([byte])!r}")
            seen |= keys
            for k in keys:
                code[k] = a
        self.alphabet = alphabet
        self.gap_open, self.gap_extend = int(gap_open), int(gap_extend)
        self.unknown = unknown
        self.case_insensitive = bool(case_insensitive)
        self.n_sym = n + 1
        self.code = code
        # (n + 1) x (n + 1): the unknown symbol's row and column
        self.table = [r + [unknown] for r in table] + [[unknown] * (n + 1)]

    @classmethod
    def from_ncbi(cls, text, gap_open: int, gap_extend: int, **kw):
        """The usual text form of a matrix: '#' comment lines, a header line of
        the symbols, then one row per symbol (the symbol, then its entries, in
        the header's order): the row's symbol is the db symbol.  A '*' row or
        column, if there is one, is not a symbol: its corner entry becomes
        ``unknown`` unless that is given."""
        if isinstance(text, bytes):
            text = text.decode("ascii")
        lines = [ln.split("#", 1)[0].split() for ln in text.splitlines()]
        lines = [ln for ln in lines if ln]
        if not lines:
            raise ValueError("SubstitutionMatrix.from_ncbi: no header line")
        header, body = lines[0], lines[1:]
        if any(len(h) != 1 or ord(h) > 127 for h in header):
            raise ValueError("SubstitutionMatrix.from_ncbi: the header must list one-byte symbols")
        if len(body) != len(header):
            raise ValueError(f"SubstitutionMatrix.from_ncbi: {len(header)} symbols in the header, "
                             f"{len(body)} rows")
        full = []
        for h, row in zip(header, body):
            if row[0] != h:
                raise ValueError(f"SubstitutionMatrix.from_ncbi: row {row[0]!r} where the header "
                                 f"has {h!r}")
            if len(row) != len(header) + 1:
                raise ValueError(f"SubstitutionMatrix.from_ncbi: row {h!r} has {len(row) - 1} "
                                 f"entries, the header {len(header)} symbols")
            try:
                full.append([int(v) for v in row[1:]])
            except ValueError:
                raise ValueError(f"SubstitutionMatrix.from_ncbi: row {h!r} holds a non-integer") from None
        keep = [k for k, h in enumerate(header) if h != "*"]
        if len(keep) < len(header) and "unknown" not in kw:
            star = header.index("*")
            kw["unknown"] = full[star][star]
        alphabet = "".join(header[k] for k in keep).encode("ascii")
        return cls(alphabet, [[full[a][b] for b in keep] for a in keep], gap_open, gap_extend, **kw)

    def s(self, db_byte: int, q_byte: int) -> int:
        """The score of one db byte against one query byte."""
        return self.table[self.code[db_byte]][self.code[q_byte]]

    def c_struct(self) -> "_lib.SubMatrix":
        """The saln_sub_matrix of this matrix."""
        m = _lib.SubMatrix()
        m.n_sym = self.n_sym
        m.gap_open, m.gap_extend = self.gap_open, self.gap_extend
        for b in range(256):
            m.code[b] = self.code[b]
        for a, row in enumerate(self.table):
            for b, v in enumerate(row):
                m.score[a][b] = v
        return m

    def check(self) -> int:
        """saln_sub_matrix_check (host only): raises SalnError outside the
        engine's domain; returns the range guard's largest |parameter|."""
        mx = C.c_int32()
        _lib.check(_lib.lib().saln_sub_matrix_check(C.byref(self.c_struct()), C.byref(mx)),
                   "saln_sub_matrix_check")
        return mx.value


def _scoring_entry(entry: str, scoring):
    """(entry point, scoring argument): the saln_ends_free_sub_* form of
    `entry` under a SubstitutionMatrix, `entry` itself under a 4-tuple."""
    if isinstance(scoring, SubstitutionMatrix):
        return entry.replace("saln_ends_free_", "saln_ends_free_sub_", 1), C.pointer(scoring.c_struct())
    return entry, _lib.scoring_arg(scoring)


def _xdrop_entry(entry: str, mode, xdrop):
    """(entry point, the arguments between the pair count and the scoring, those
    after it): `entry` with its mode, or with xdrop (an int: EXTEND only) its
    saln_ends_free_xdrop_* form, which takes no mode and X after the scoring."""
    if xdrop is None:
        return entry, (_mode(mode),), ()
    if _mode(mode) != EXTEND:
        raise ValueError("xdrop is part of extension alignment: mode must be EXTEND")
    if isinstance(xdrop, bool) or int(xdrop) != xdrop:
        raise ValueError(f"xdrop {xdrop!r} is not an integer")
    return entry.replace("saln_ends_free_", "saln_ends_free_xdrop_", 1), (), (int(xdrop),)


def xdrop_steps(results):
    """The row-loop steps each pair's group of lanes ran under ``xdrop=`` (the
    records' ``reserved``; 0 without xdrop): a diagnostic that, unlike the rest
    of a record, depends on the class geometry.  At most min(m, L) + lanes,
    L the last db row with an unpruned cell; a plain fill runs m + lanes - 1."""
    return results["reserved"]


def _mode(mode) -> int:
    if isinstance(mode, Mode):
        return {Mode.Global: 0, Mode.Local: 1, Mode.SemiGlobal: 2}[mode]
    return int(mode)


def _pair_lists(pairs, n_q, n_db):
    if pairs is None:
        return None, None, n_q * n_db
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]), len(pairs)


def _align_batch(entry, queries, dbs, pairs, mode, scoring, trace_budget, cigar, device, xdrop=None):
    """saln_ends_free_align_batch or saln_ends_free_long_align_batch (entry)."""
    entry, mode_arg, x_arg = _xdrop_entry(entry, mode, xdrop)
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    pq, pd, n = _pair_lists(pairs, len(qo) - 1, len(do) - 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    L = _lib.lib()
    h = C.c_void_p()
    entry, sarg = _scoring_entry(entry, scoring)
    _lib.check(getattr(L, entry)(
        _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq),
        vp(pd), n, *mode_arg, sarg, *x_arg, int(trace_budget), int(bool(cigar)),
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
                          cigar: bool = True, device: int = 0, xdrop=None):
    """Local, semi-global, overlap (mode=OVERLAP) or extension (mode=EXTEND)
    alignment of a batch.
    pairs: None (all-vs-all, db
    outer / query inner) or (n, 2) (query index, db index).  Returns (results,
    cigars): results is a structured array (score, status, q_begin, q_end,
    db_begin, db_end, cigar_len; the ranges half-open and 0-based), cigars a
    CigarBatch (pair k's [(length, op), ...]).  cigar=False runs the fill only:
    score and ends, begins -1, no words.  A pair whose trace codes alone exceed
    trace_budget bytes (0 selects 1 GiB per chunk) has status TRACE_CAP, its
    score and ends, begins -1 and no words.  xdrop: None, or X >= 0 with
    mode=EXTEND (ValueError under another mode): the X-drop extension, whose
    records carry the fill's steps in ``reserved``."""
    return _align_batch("saln_ends_free_align_batch", queries, dbs, pairs, mode, scoring,
                        trace_budget, cigar, device, xdrop)


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


def _int_xdrop(xdrop) -> int:
    if isinstance(xdrop, bool) or not isinstance(xdrop, (int, np.integer)):
        raise ValueError(f"xdrop {xdrop!r} is not an integer")
    return int(xdrop)


def xdrop_extend_long_batch(queries, dbs, pairs=None, *, xdrop, scoring=None, trace_budget: int = 0,
                            cigar: bool = True, device: int = 0, replay: bool = False):
    """X-drop extension (mode EXTEND with ``xdrop`` = X >= 0, the module's text)
    of a batch of pairs of any length (saln_ends_free_xdrop_long_align_batch):
    ends_free_align_batch(..., mode=EXTEND, xdrop=X) without the length limits,
    with the same arguments and return.  A pair of at most 1,024 x 65,000 runs
    the same fill as there and gives the same record, steps included; every
    other pair runs the chunked X-drop fill, and its ``reserved`` holds the
    row-loop steps summed over the chunks it ran (``xdrop_steps``).  The only
    limit is the range guard, (n + m + 2) * max|parameter| + X < 2^30.  Codes
    are sized as under ends_free_align_long_batch (``trace_bytes_long``).
    replay=True (saln_ends_free_xdrop_replay_align_batch): the same records
    (``reserved`` may differ: the forward pass's steps) and words, but a pair
    of the chunked fill holds ``xdrop_replay_bytes`` against trace_budget and
    its alignment comes from the tiled replay (option ``ends_free.tile_rows``);
    TRACE_CAP then means that this replay footprint alone exceeds the budget."""
    entry = "saln_ends_free_replay_align_batch" if replay else "saln_ends_free_long_align_batch"
    return _align_batch(entry, queries, dbs, pairs, EXTEND, scoring, trace_budget, cigar, device,
                        _int_xdrop(xdrop))


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


def _extend(seq1, seq2, direction, scoring, trace_budget, device, **kw):
    if direction == "right":
        return _one(seq1, seq2, EXTEND, scoring, trace_budget, device, **kw)
    if direction != "left":
        raise ValueError(f"extend_align: direction {direction!r} is neither 'right' nor 'left'")
    q, d = bytes(seq1), bytes(seq2)
    rec, cigar = _one(q[::-1], d[::-1], EXTEND, scoring, trace_budget, device, **kw)
    rec = rec.copy()
    rec["q_begin"], rec["q_end"] = len(q) - int(rec["q_end"]), len(q)
    rec["db_begin"], rec["db_end"] = len(d) - int(rec["db_end"]), len(d)
    return rec, list(cigar)[::-1]


def extend_align(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0,
                 direction: str = "right", xdrop=None):
    """(result record, cigar) of the best extension of seq1 (query) and seq2
    (db) from an anchor: the alignment of a prefix seq1[:q_end] with a prefix
    seq2[:db_end] that scores highest, q_begin = db_begin = 0; score 0 and no
    words when no such pair scores above 0.

    direction="left" extends leftwards from an anchor at the sequences' ends:
    the same kernels run on both sequences reversed, the CIGAR comes back
    reversed (so it reads left to right along the sequences as given), and
    the coordinates are counted on the sequences as given, from their right
    ends: with (q_end', db_end') the end cell of the reversed run,
    q_begin = len(seq1) - q_end', q_end = len(seq1), db_begin = len(seq2) -
    db_end', db_end = len(seq2); the alignment is seq1[q_begin:] against
    seq2[db_begin:], and the empty one has q_begin = q_end = len(seq1).  A
    SubstitutionMatrix is not transposed by it: its rows stay the db's
    symbols.  alignment_score takes the result of either direction.

    xdrop=X: the X-drop extension (the module's text), in either direction;
    leftwards the drop-off is counted from the anchor at the right ends."""
    kw = {} if xdrop is None else {"xdrop": xdrop}
    return _extend(seq1, seq2, direction, scoring, trace_budget, device, **kw)


def extend_align_long(seq1, seq2, *, scoring=None, trace_budget: int = 0, device: int = 0,
                      direction: str = "right", replay: bool = False):
    """extend_align for sequences of any length (ends_free_align_long_batch)."""
    return _extend(seq1, seq2, direction, scoring, trace_budget, device,
                   batch=ends_free_align_long_batch, replay=replay)


def xdrop_extend_long(seq1, seq2, *, xdrop, scoring=None, trace_budget: int = 0, device: int = 0,
                      direction: str = "right", replay: bool = False):
    """extend_align(..., xdrop=X) for sequences of any length
    (xdrop_extend_long_batch); direction="left" as there.  replay=True: the
    tiled replay, as there; TRACE_CAP then means the replay footprint
    (``xdrop_replay_bytes``) exceeds trace_budget."""
    def batch(qs, ds, pairs, *, mode, **kw):
        return xdrop_extend_long_batch(qs, ds, pairs, **kw)
    return _extend(seq1, seq2, direction, scoring, trace_budget, device, batch=batch,
                   xdrop=_int_xdrop(xdrop), replay=replay)


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


def alignment_score(q, d, result_or_cigar, scoring=None, q_begin=None, db_begin=None) -> int:
    """The score of an alignment recomputed from the sequences: q (query) and
    d (db) as bytes, the alignment as its CIGAR ([(n, op)]) with q_begin and
    db_begin, or as (result record, cigar) as the one-pair functions return it
    (the begins then come from the record).  scoring: the 4-tuple or a
    SubstitutionMatrix; under a matrix a column scores by its two bytes, which
    cigar_score cannot know."""
    if (isinstance(result_or_cigar, tuple) and len(result_or_cigar) == 2
            and getattr(getattr(result_or_cigar[0], "dtype", None), "names", None)):
        rec, cigar = result_or_cigar
        q_begin = int(rec["q_begin"]) if q_begin is None else q_begin
        db_begin = int(rec["db_begin"]) if db_begin is None else db_begin
    else:
        cigar = result_or_cigar
    j, i = int(q_begin or 0), int(db_begin or 0)
    q, d = bytes(q), bytes(d)
    if isinstance(scoring, SubstitutionMatrix):
        o, e, s = scoring.gap_open, scoring.gap_extend, scoring.s
    else:
        m, x, o, e = scoring if scoring is not None else DEFAULT_SCORING
        s = lambda a, b: m if a == b else x  # noqa: E731
    total, prev = 0, None
    for n, op in cigar:
        if op in "=X":
            if j + n > len(q) or i + n > len(d):
                raise ValueError("alignment_score: the alignment runs past a sequence's end")
            for k in range(n):
                if (q[j + k] == d[i + k]) != (op == "="):
                    raise ValueError(f"alignment_score: '{op}' at query {j + k}, db {i + k} does not "
                                     "agree with the bytes")
                total += s(d[i + k], q[j + k])
            i, j = i + n, j + n
        elif op == "I":
            total += e * n + (o if op != prev else 0)
            j += n
        elif op == "D":
            total += e * n + (o if op != prev else 0)
            i += n
        else:
            raise ValueError(f"alignment_score: unknown op {op!r}")
        prev = op
    if j > len(q) or i > len(d):
        raise ValueError("alignment_score: the alignment runs past a sequence's end")
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


def xdrop_replay_bytes(len_q: int, len_db: int, tile_rows: int = 0) -> int:
    """saln_ends_free_xdrop_replay_bytes: bytes one pair holds against
    trace_budget under xdrop_extend_long_batch(..., replay=True) (host only).
    trace_bytes within the class limits; above them a header per chunk, the
    boundary columns and the checkpoint rows (16 bytes per entry: B is kept
    too) and one tile of codes, sized for all rows.  tile_rows 0: the value of
    option ends_free.tile_rows."""
    out = C.c_uint64()
    _lib.check(_lib.lib().saln_ends_free_xdrop_replay_bytes(int(len_q), int(len_db), int(tile_rows),
                                                            C.byref(out)),
               "saln_ends_free_xdrop_replay_bytes")
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


def fill_geometry(len_q: int, ld_max: int, has_matrix: bool = False) -> tuple[int, int]:
    """saln_ends_free_fill_geometry: (lane groups per workgroup, bytes of LDS
    their staged db rows take) of the class fill that runs queries of len_q
    columns in a launch whose longest db has ld_max rows (host only);
    has_matrix: under a SubstitutionMatrix, whose block shares the 64 KB.  A
    workgroup has groups * pair_geometry(len_q)[0] lanes.  Raises SalnError
    (E_INVALID) above MAX_QUERY columns or 65,000 rows."""
    groups, lds = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().saln_ends_free_fill_geometry(int(len_q), int(ld_max), int(bool(has_matrix)),
                                                       C.byref(groups), C.byref(lds)),
               "saln_ends_free_fill_geometry")
    return groups.value, lds.value


def _score_limits(scoring):
    """(S+, A) of a scoring for score_path: the largest positive s(i, j) and
    the largest |parameter|, gaps included."""
    if isinstance(scoring, SubstitutionMatrix):
        flat = [v for r in scoring.table for v in r]
        return max(0, max(flat)), scoring.check()
    sc = tuple(int(v) for v in (scoring if scoring is not None else DEFAULT_SCORING))
    return max(0, sc[0]), max(abs(v) for v in sc)


def score_path(len_q: int, len_db: int, mode, scoring=None) -> bool:
    """saln_ends_free_score_path (host only): does a pair of len_q columns and
    len_db rows run the packed-i16 fill of score_batch / EndsFreeScorePlan
    under this mode and scoring (the 4-tuple or a SubstitutionMatrix)?  Local
    and semi-global only, and only while min(n, m) * S+ + 4 * A < 2^15 and, in
    semi-global, (n + 4) * A < 2^15; every other pair runs the i32 fill.  Option
    ``ends_free.score_i16`` = 0 sends every pair there and is not counted here.
    Raises SalnError (E_INVALID) above MAX_QUERY columns or 65,000 rows."""
    pos, mx = _score_limits(scoring)
    out = C.c_int32()
    _lib.check(_lib.lib().saln_ends_free_score_path(int(len_q), int(len_db), _mode(mode), pos, mx,
                                                    C.byref(out)), "saln_ends_free_score_path")
    return bool(out.value)


def score_geometry(len_q: int, ld_max: int, has_matrix: bool = False) -> tuple[int, int]:
    """saln_ends_free_score_geometry (host only): (lane groups per workgroup,
    two pairs each; bytes of LDS their staged db rows take) of the packed fill
    that runs queries of len_q columns in a launch whose longest db has ld_max
    rows: fill_geometry's rule over rows of twice the bytes."""
    groups, lds = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().saln_ends_free_score_geometry(int(len_q), int(ld_max), int(bool(has_matrix)),
                                                        C.byref(groups), C.byref(lds)),
               "saln_ends_free_score_geometry")
    return groups.value, lds.value


def score_batch(queries, dbs, pairs=None, *, mode, scoring=None, device: int = 0) -> np.ndarray:
    """The scores of a batch and nothing else (saln_ends_free_score_batch): the
    first step of a search, before the few pairs that matter are aligned.
    Returns int32[n_pairs]: exactly the ``score`` that ends_free_align_batch
    gives each pair under the same mode (any of the four) and scoring (the
    4-tuple or a SubstitutionMatrix).  pairs as there.  Local and semi-global
    pairs whose values fit 16 bits (score_path) run two to a lane group in the
    packed fill; every other pair runs the i32 fill.  Limits: MAX_QUERY columns
    and 65,000 rows."""
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    pq, pd, n = _pair_lists(pairs, len(qo) - 1, len(do) - 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    entry, sarg = _scoring_entry("saln_ends_free_score_batch", scoring)
    scores = np.zeros(max(n, 1), np.int32)
    _lib.check(getattr(_lib.lib(), entry)(
        _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq), vp(pd), n,
        _mode(mode), sarg, scores.ctypes.data_as(C.POINTER(C.c_int32))), entry)
    return scores[:n]


class EndsFreeScorePlan:
    """Device-resident score search (saln_ends_free_score_plan_create): plan
    from host offsets and a pair list once, execute any number of times on
    device (torch) sequence buffers into a device int32 tensor of n_pairs
    scores, each the ``score`` of ends_free_align_batch.  scoring: the 4-tuple
    or a SubstitutionMatrix.  ``info()``: how many pairs run the packed-i16 fill
    and how many the i32 fill (score_path; option ``ends_free.score_i16`` = 0,
    read when the plan is created, sends all to i32).  The plan owns the i32
    pairs' workspace: its executes must not overlap."""

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
        entry, sarg = _scoring_entry("saln_ends_free_score_plan_create", scoring)
        _lib.check(getattr(L, entry)(_lib.context(device), vp(qo), len(qo) - 1, vp(do), len(do) - 1,
                                     vp(pq), vp(pd), n, _mode(mode), sarg, C.byref(self._h)), entry)

    def execute(self, d_q, d_db, d_scores, stream=None):
        """d_q / d_db: device uint8 tensors (CSR bytes), d_scores: device
        int32[n_pairs]."""
        assert d_scores.numel() * d_scores.dtype.itemsize >= 4 * self.n_pairs
        if stream is None:  # torch's current stream, like EndsFreePlan.execute
            stream = _lib.torch_stream(d_scores.device)
        _lib.check(self._L.saln_ends_free_score_execute(
            self._h, C.c_void_p(d_q.data_ptr()), C.c_void_p(d_db.data_ptr()),
            C.c_void_p(d_scores.data_ptr()), C.c_void_p(stream)), "saln_ends_free_score_execute")

    def info(self) -> tuple[int, int]:
        """(pairs of the packed fill, pairs of the i32 fill)."""
        pk, i32 = C.c_uint64(), C.c_uint64()
        _lib.check(self._L.saln_ends_free_score_plan_info(self._h, C.byref(pk), C.byref(i32)),
                   "saln_ends_free_score_plan_info")
        return pk.value, i32.value

    def close(self):
        if self._h:
            self._L.saln_ends_free_score_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EndsFreePlan:
    """Device-resident score-only batch: plan from host offsets and a pair
    list once, execute on device (torch) sequence buffers into a device tensor
    of result records (n_pairs x 8 int32: score, status, q_begin = -1, q_end,
    db_begin = -1, db_end, 0, 0).  scoring: the 4-tuple or a SubstitutionMatrix
    (saln_ends_free_sub_plan_create: the database-search shape).  xdrop: None,
    or X >= 0 with mode=EXTEND: the X-drop extension
    (saln_ends_free_xdrop_plan_create), the last int32 then the fill's steps."""

    def __init__(self, q_off, db_off, pairs=None, *, mode, scoring=None, device: int = 0, xdrop=None):
        L = _lib.lib()
        self._L = L
        self.device = device
        qo = np.ascontiguousarray(q_off, np.uint64)
        do = np.ascontiguousarray(db_off, np.uint64)
        pq, pd, n = _pair_lists(pairs, len(qo) - 1, len(do) - 1)
        self.n_pairs = n
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._h = C.c_void_p()
        entry, mode_arg, x_arg = _xdrop_entry("saln_ends_free_plan_create", mode, xdrop)
        entry, sarg = _scoring_entry(entry, scoring)
        _lib.check(getattr(L, entry)(_lib.context(device), vp(qo), len(qo) - 1, vp(do), len(do) - 1,
                                     vp(pq), vp(pd), n, *mode_arg, sarg, *x_arg, C.byref(self._h)), entry)

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
