"""NW-affine engine, Python face of the C ABI.

Mirrors ``pub fn n_w_align(seq1: &Record, seq2: &Record, _verbose: bool,
mode: Mode) -> Result<()>`` (src/needleman_wunsch_affine.rs:424-437): seq1 is
the query, seq2 the db record; non-global modes raise
``AlignmentError("not implemented")`` like :433-434.  Where the reference
only prints, this returns the score, the reference's would-be panic as a
status, and the first printed alignment as a CIGAR; ``render`` produces the
reference's exact text.  All compute runs in libsaln's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence
from dataclasses import dataclass

import numpy as np

from . import _lib
from .records import AlignmentError, Mode, Record

DEFAULT_SCORING = (5, -4, -8, -6)  # SCHEME, needleman_wunsch_affine.rs:15-20


@dataclass
class NwAlignment:
    score: int
    status: int                     # _lib.OK / REF_PANIC_BOUNDARY
    end_states: int                 # bit0 M, bit1 I, bit2 D
    printed: bool                   # the reference prints >= 1 block
    cigar: list[tuple[int, str]]    # first printed alignment, forward order

    @property
    def panics(self) -> bool:
        return self.status == _lib.REF_PANIC_BOUNDARY

    @property
    def cigar_str(self) -> str:
        return "".join(f"{n}{op}" for n, op in self.cigar)


def _decode_cigar(words) -> list[tuple[int, str]]:
    return [(int(w) >> 4, _lib.CIGAR_OPS[int(w) & 15]) for w in words]


class CigarBatch(Sequence):
    """The first printed alignments of a batch, decoded on access: item k is
    pair k's CIGAR as [(length, op), ...] (op in '=', 'X', 'I', 'D'); words(k)
    is its raw (length << 4 | op) words.  Indexable, iterable and comparable
    like the list it stands for, without building ~30 tuples per pair up
    front (10^5 pairs: ~1.3 s in Python)."""

    def __init__(self, words: np.ndarray, offsets: np.ndarray, lengths: np.ndarray):
        self._w, self._o, self._n = words, offsets, lengths

    def __len__(self) -> int:
        return len(self._n)

    def words(self, k: int) -> np.ndarray:
        o = int(self._o[k])
        return self._w[o:o + int(self._n[k])]

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        return _decode_cigar(self.words(k))

    def __eq__(self, other) -> bool:
        if not isinstance(other, Sequence) or isinstance(other, (str, bytes)):
            return NotImplemented
        return len(self) == len(other) and all(self[k] == other[k] for k in range(len(self)))

    def __ne__(self, other) -> bool:
        eq = self.__eq__(other)
        return eq if eq is NotImplemented else not eq

    __hash__ = None

    def tolist(self) -> list:
        """A real list of every pair's CIGAR (for json.dumps, isinstance checks)."""
        return [self[k] for k in range(len(self))]

    def __add__(self, other) -> list:
        return self.tolist() + list(other)

    def __radd__(self, other) -> list:
        return list(other) + self.tolist()


def cigar_ops_string(cigar: list[tuple[int, str]]) -> str:
    """Expanded one-char-per-column op string ('=', 'X', 'I', 'D')."""
    return "".join(op * n for n, op in cigar)


def alignment_rows(query: bytes, db: bytes, cigar: list[tuple[int, str]]) -> tuple[str, str, str]:
    """(seq1 line, bar line, seq2 line) of an alignment, TraceBackInfo Display :390-411."""
    i = j = 0
    s1, s2 = [], []
    for n, op in cigar:
        for _ in range(n):
            if op in "=X":
                s1.append(chr(query[j])); s2.append(chr(db[i])); i += 1; j += 1
            elif op == "I":
                s1.append(chr(query[j])); s2.append("-"); j += 1
            else:
                s1.append("-"); s2.append(chr(db[i])); i += 1
    bars = "".join("|" if a == b else " " for a, b in zip(s1, s2))
    return "".join(s1), bars, "".join(s2)


def _bytes(x) -> bytes:
    if isinstance(x, Record):
        return x.seq
    return bytes(x)


def n_w_align(seq1, seq2, verbose: bool = False, mode: Mode = Mode.Global, *, scoring=None,
              device: int = 0) -> NwAlignment:
    """needleman_wunsch_affine.rs:424 — seq1 = query, seq2 = db (Record or bytes)."""
    q, d = _bytes(seq1), _bytes(seq2)
    L = _lib.lib()
    ctx = _lib.context(device)
    res = _lib.NwResult()
    cap = len(q) + len(d) + 1
    cig = (C.c_uint32 * cap)()
    qb = C.create_string_buffer(q, len(q)) if q else None
    db = C.create_string_buffer(d, len(d)) if d else None
    rc = L.saln_nw_align(ctx, qb, len(q), db, len(d), int(verbose), int(mode),
                         _lib.scoring_arg(scoring), C.byref(res), cig, cap)
    if rc == _lib.NOT_IMPLEMENTED:
        raise AlignmentError("not implemented")
    _lib.check(rc, "saln_nw_align")
    return NwAlignment(res.score, res.status, res.end_states, bool(res.printed),
                       _decode_cigar(cig[:res.cigar_len]))


def render(seq1, seq2, mode: Mode = Mode.Global, max_blocks: int = 0, *,
           device: int = 0) -> tuple[str, int, int]:
    """Reference stdout for one pair (timing line excluded): (text, blocks,
    status); one library call (saln_nw_render_text)."""
    q, d = _bytes(seq1), _bytes(seq2)
    L = _lib.lib()
    qb = C.create_string_buffer(q, len(q)) if q else None
    db = C.create_string_buffer(d, len(d)) if d else None
    h = C.c_void_p()
    _lib.check(L.saln_nw_render_text(_lib.context(device), qb, len(q), db, len(d), int(mode),
                                     max_blocks, C.byref(h)), "saln_nw_render_text")
    try:
        text, blocks, status, _ = _text_get(h, 0)
    finally:
        L.saln_nw_text_free(h)
    if status == _lib.NOT_IMPLEMENTED:
        raise AlignmentError("not implemented")
    return text, blocks, status


def _text_get(h, k: int):
    ptr, n, nb, st, ns = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int32(), C.c_uint64()
    _lib.check(_lib.lib().saln_nw_text_get(h, k, C.byref(ptr), C.byref(n), C.byref(nb),
                                           C.byref(st), None, C.byref(ns)), "saln_nw_text_get")
    text = C.string_at(ptr.value, n.value).decode("latin-1") if n.value else ""
    return text, nb.value, st.value, ns.value


def render_batch(queries, dbs, pairs=None, *, mode: Mode = Mode.Global, max_blocks: int = 0,
                 stop_at_panic: bool = False, device: int = 0,
                 stats: dict | None = None) -> list[tuple[str, int, int]]:
    """The reference's stdout per pair of a batch (saln_nw_render_batch: one
    plan, every pair computed once): [(text, blocks, status)] in pair order
    (pairs=None: all-vs-all, db outer / query inner, main.rs:61-62).  With
    stop_at_panic the list ends at the first pair whose traceback panics (the
    reference aborts there).  stats (a dict) receives "gpu_decided": the pairs
    rendered from the GPU's walk alone."""
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    if pairs is None:
        pq = pd = None
        n = len(queries) * len(dbs)
    else:
        pa = np.asarray(pairs, np.uint32).reshape(-1, 2)
        pq, pd = np.ascontiguousarray(pa[:, 0]), np.ascontiguousarray(pa[:, 1])
        n = len(pa)
    L = _lib.lib()
    h = C.c_void_p()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None  # noqa: E731
    _lib.check(L.saln_nw_render_batch(_lib.context(device), ptr(qs), ptr(qo), len(queries),
                                      ptr(ds), ptr(do), len(dbs), ptr(pq), ptr(pd), n, int(mode),
                                      max_blocks, 1 if stop_at_panic else 0, C.byref(h)),
               "saln_nw_render_batch")
    try:
        if stats is not None:
            stats["gpu_decided"] = int(L.saln_nw_text_gpu_decided(h))
        return [_text_get(h, k)[:3] for k in range(L.saln_nw_text_count(h))]
    finally:
        L.saln_nw_text_free(h)


def dense_mask(seq1, seq2, scoring=None, *, device: int = 0) -> np.ndarray:
    """(len_db+1, len_q+1) uint8 parent codes (include/saln.h saln_nw_dense_mask)."""
    q, d = _bytes(seq1), _bytes(seq2)
    out = np.zeros((len(d) + 1, len(q) + 1), np.uint8)
    qb = C.create_string_buffer(q, len(q)) if q else None
    db = C.create_string_buffer(d, len(d)) if d else None
    _lib.check(_lib.lib().saln_nw_dense_mask(_lib.context(device), qb, len(q), db, len(d),
                                             _lib.scoring_arg(scoring),
                                             out.ctypes.data_as(C.c_void_p)),
               "saln_nw_dense_mask")
    return out


def pack_csr(seqs) -> tuple[np.ndarray, np.ndarray]:
    """list of bytes -> (uint8 concatenation, uint64 offsets[n+1])."""
    seqs = [_bytes(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(seqs), np.uint8) if off[-1] else np.zeros(1, np.uint8)
    return np.ascontiguousarray(buf), off


def nw_align_batch(queries, dbs, pairs=None, mode: Mode = Mode.Global, *, scoring=None,
                   device: int = 0, with_cigar: bool = True, ctx=None):
    """Batched n_w_align.  pairs: None (all-vs-all, db outer / query inner like
    main.rs:61-62) or an (n, 2) array of (query index, db index).  ctx: a
    context of the caller's (_lib.new_context) instead of the per-process one.
    Returns (results structured array, CIGARs or None): the CIGARs are a
    CigarBatch, pair k's [(length, op), ...] decoded when read."""
    qs, qo = pack_csr(queries)
    ds, do = pack_csr(dbs)
    if pairs is None:
        n = len(qo) - 1
        n_pairs = n * (len(do) - 1)
        pq = pd = None
    else:
        pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
        n_pairs = len(pairs)
        pq = np.ascontiguousarray(pairs[:, 0])
        pd = np.ascontiguousarray(pairs[:, 1])
    res = np.zeros(n_pairs, dtype=_lib.RESULT_DTYPE)
    if n_pairs == 0:
        return res, ([] if with_cigar else None)
    lq = np.diff(qo).astype(np.int64)
    ld = np.diff(do).astype(np.int64)
    if pairs is None:
        per = np.add.outer(ld, lq).reshape(-1)
    else:
        per = lq[pq] + ld[pd]
    coff = np.zeros(n_pairs + 1, np.uint64)
    coff[1:] = np.cumsum(per, dtype=np.uint64)
    cig = np.zeros(max(1, int(coff[-1])), np.uint32) if with_cigar else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    rc = _lib.lib().saln_nw_align_batch(
        ctx if ctx is not None else _lib.context(device), vp(qs), vp(qo), len(qo) - 1, vp(ds), vp(do), len(do) - 1, vp(pq),
        vp(pd), n_pairs, int(mode), _lib.scoring_arg(scoring), vp(res), vp(cig), vp(coff))
    if rc == _lib.NOT_IMPLEMENTED:
        raise AlignmentError("not implemented")
    _lib.check(rc, "saln_nw_align_batch")
    cigars = CigarBatch(cig, coff[:-1], res["cigar_len"].copy()) if with_cigar else None
    return res, cigars


@dataclass(frozen=True)
class PairPath:
    variant: int      # fill variant number; -1: a pair with an empty side
    packed: bool      # int16 halves (two pairs per lane group) or i32 lanes
    rebase: bool      # the packed launch uses the rebasing int16 frame
    table: int        # packed launch body: 0 generic, 2 / 4 table at that scale, 3 row profiles
    stripe_pk: bool   # column-stripe pairs: packed stripes
    rows_k: int       # column-stripe pairs: the row fill's columns per lane


class NwPlan:
    """Device-resident batch: plan once from host lengths, execute on torch
    device tensors (inputs resident in HBM).  Used by bench.py and the
    multi-GPU driver."""

    def __init__(self, q_off: np.ndarray, db_off: np.ndarray, pairs=None, *, scoring=None,
                 device: int = 0, ctx=None, full_codes: bool = False):
        """full_codes: the fills store the reference's full parent sets (1 B
        per cell, saln_nw_plan_create_full) instead of walk codes."""
        self._L = _lib.lib()
        self.full_codes = bool(full_codes)
        self.device = device
        self.q_off = np.ascontiguousarray(q_off, np.uint64)
        self.db_off = np.ascontiguousarray(db_off, np.uint64)
        n_q, n_db = len(self.q_off) - 1, len(self.db_off) - 1
        if pairs is None:
            self.n_pairs = n_q * n_db
            pq = pd = None
        else:
            pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
            self.n_pairs = len(pairs)
            pq = np.ascontiguousarray(pairs[:, 0])
            pd = np.ascontiguousarray(pairs[:, 1])
        self._h = C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        ctx = ctx if ctx is not None else _lib.context(device)
        create = (self._L.saln_nw_plan_create_full if self.full_codes
                  else self._L.saln_nw_plan_create)
        _lib.check(create(ctx, vp(self.q_off), n_q, vp(self.db_off), n_db, vp(pq), vp(pd),
                          self.n_pairs, int(Mode.Global), _lib.scoring_arg(scoring),
                          C.byref(self._h)),
                   "saln_nw_plan_create")
        self._lens = (np.diff(self.q_off)[pq if pq is not None else
                                          np.arange(self.n_pairs) % max(1, n_q)],
                      np.diff(self.db_off)[pd if pd is not None else
                                           np.arange(self.n_pairs) // max(1, n_q)])
        mb, cw, cells = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._L.saln_nw_plan_info(self._h, C.byref(mb), C.byref(cw), C.byref(cells))
        self.mask_bytes, self.cigar_words, self.cells = mb.value, cw.value, cells.value
        self.cigar_off = np.zeros(self.n_pairs + 1, np.uint64)
        self._L.saln_nw_cigar_offsets(self._h, self.cigar_off.ctypes.data_as(C.c_void_p))

    def execute(self, q_seq, db_seq, results, cigar=None, stream=None) -> None:
        """q_seq/db_seq/results/cigar: torch CUDA tensors (uint8 / uint8 /
        int32[n_pairs*4] / int32[cigar_words]) or raw device pointers."""
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa
        if stream is None:
            stream = _lib.torch_stream(self.device)
        _lib.check(self._L.saln_nw_execute(self._h, ptr(q_seq), ptr(db_seq), ptr(results),
                                           ptr(cigar), stream), "saln_nw_execute")

    def dense_mask(self, pair: int) -> np.ndarray:
        """Pair `pair`'s parent sets from the last execute of a synchronous
        full-code plan: (len_db+1, len_q+1) uint8 (saln_nw_plan_dense_mask)."""
        lq, ld = int(self._lens[0][pair]), int(self._lens[1][pair])
        out = np.zeros((ld + 1, lq + 1), np.uint8)
        _lib.check(self._L.saln_nw_plan_dense_mask(self._h, pair, out.ctypes.data_as(C.c_void_p)),
                   "saln_nw_plan_dense_mask")
        return out

    def walk_codes(self, pair: int) -> np.ndarray:
        """Pair `pair`'s 4-bit walk codes from the last execute of a synchronous
        plan: (len_db, len_q) uint8, bits set = parent absent (0 argI, 1 argD,
        2 I-open, 3 D-open; argM at the end cell), saln_nw_plan_walk_codes."""
        lq, ld = int(self._lens[0][pair]), int(self._lens[1][pair])
        out = np.zeros((ld, lq), np.uint8)
        _lib.check(self._L.saln_nw_plan_walk_codes(self._h, pair, out.ctypes.data_as(C.c_void_p)),
                   "saln_nw_plan_walk_codes")
        return out

    def pair_path(self, pair: int) -> "PairPath":
        """What the next execute does with pair `pair` (test introspection,
        saln_nw_plan_pair_path): the fill variant and, from the code that
        launches it, the frame and body of its launch."""
        pp = _lib.NwPairPath()
        _lib.check(self._L.saln_nw_plan_pair_path(self._h, pair, C.byref(pp)),
                   "saln_nw_plan_pair_path")
        return PairPath(pp.variant, bool(pp.packed), bool(pp.rebase), pp.table,
                        bool(pp.stripe_pk), pp.rows_k)

    def status(self) -> int:
        """Wait for every execute since the last call; return and clear the
        device error flags they raised (include/saln.h saln_nw_plan_status)."""
        f = C.c_uint32()
        rc = self._L.saln_nw_plan_status(self._h, C.byref(f))
        if rc not in (_lib.OK, _lib.E_DEVICE_WAIT):
            _lib.check(rc, "saln_nw_plan_status")
        return f.value

    def check(self) -> None:
        """Raise SalnError(E_DEVICE_WAIT) if any execute since the last
        check/status hit a device-side dependency timeout: its results are
        invalid.  Blocks until those executes finish."""
        _lib.check(self._L.saln_nw_plan_status(self._h, None), "NwPlan execute (device status)")

    def set_wait_limit(self, polls: int) -> None:
        """Polls a column-stripe dependency wait may spend (test hook: 0
        injects a timeout on any wait that finds its row unpublished)."""
        _lib.check(self._L.saln_nw_plan_set_wait_limit(self._h, polls), "set_wait_limit")

    def set_async(self, enable: bool) -> None:
        """2-deep pipeline: traceback of execute n overlaps the fill of n+1."""
        _lib.check(self._L.saln_nw_plan_set_async(self._h, int(enable)), "set_async")

    def sync(self, stream=None, keep_latest: bool = False) -> None:
        """Make `stream` wait for the pending tracebacks (all, or all but the latest)."""
        if stream is None:
            stream = _lib.torch_stream(self.device)
        _lib.check(self._L.saln_nw_plan_sync(self._h, stream, int(keep_latest)), "sync")

    def set_score_only(self, enable: bool) -> None:
        """Score + panic status only: no parent codes, no traceback (C5)."""
        _lib.check(self._L.saln_nw_plan_set_score_only(self._h, int(enable)), "set_score_only")

    def set_timing(self, enable: bool) -> None:
        _lib.check(self._L.saln_nw_plan_set_timing(self._h, int(enable)), "set_timing")

    def kernel_time(self, name: str) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        self._L.saln_nw_plan_kernel_time(self._h, name.encode(), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def close(self) -> None:
        if self._h:
            self._L.saln_nw_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NwAllVsAll:
    """Score-only all-vs-all on the device (include/saln.h saln_nw_avsa_*):
    every (db d, query q) pair of the reference loop (src/main.rs:61-67),
    score + panic status at out[d, q] — the configs[4] (C5) workload.  Built
    once from host offsets; execute takes device sequences and a device
    int32[n_db * n_q * 2] output."""

    def __init__(self, q_off: np.ndarray, db_off: np.ndarray, *, scoring=None, device: int = 0):
        self._L = _lib.lib()
        self.device = device
        self.q_off = np.ascontiguousarray(q_off, np.uint64)
        self.db_off = np.ascontiguousarray(db_off, np.uint64)
        self.n_q, self.n_db = len(self.q_off) - 1, len(self.db_off) - 1
        self._h = C.c_void_p()
        _lib.check(self._L.saln_nw_avsa_create(
            _lib.context(device), self.q_off.ctypes.data_as(C.c_void_p), self.n_q,
            self.db_off.ctypes.data_as(C.c_void_p), self.n_db, int(Mode.Global),
            _lib.scoring_arg(scoring), C.byref(self._h)), "saln_nw_avsa_create")
        cells, fb = C.c_uint64(), C.c_uint64()
        self._L.saln_nw_avsa_info(self._h, C.byref(cells), C.byref(fb))
        self.cells, self.fallback_pairs = cells.value, fb.value

    def execute(self, q_seq, db_seq, out, stream=None) -> None:
        ptr = lambda t: t if isinstance(t, int) else t.data_ptr()  # noqa: E731
        if stream is None:
            stream = _lib.torch_stream(self.device)
        _lib.check(self._L.saln_nw_avsa_execute(self._h, ptr(q_seq), ptr(db_seq), ptr(out),
                                                stream), "saln_nw_avsa_execute")

    def check(self) -> None:
        """Raise SalnError(E_DEVICE_WAIT) if an execute since the last check
        hit a device-side dependency timeout (the internal plan's column
        stripes; saln_nw_avsa_status).  Blocks until those executes finish."""
        _lib.check(self._L.saln_nw_avsa_status(self._h, None), "NwAllVsAll execute (device status)")

    def close(self) -> None:
        if self._h:
            self._L.saln_nw_avsa_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nw_score_all_vs_all(queries, dbs, *, scoring=None, device: int = 0):
    """(scores, statuses), each int32[n_db, n_q] in the reference order, for
    host sequences; runs NwAllVsAll on `device`."""
    import torch
    q_seq, q_off = pack_csr(queries)
    d_seq, d_off = pack_csr(dbs)
    a = NwAllVsAll(q_off, d_off, scoring=scoring, device=device)
    dev = torch.device("cuda", device)
    tq = torch.from_numpy(q_seq.copy()).to(dev)
    td = torch.from_numpy(d_seq.copy()).to(dev)
    out = torch.empty(max(1, a.n_q * a.n_db * 2), dtype=torch.int32, device=dev)
    a.execute(tq, td, out)
    a.check()
    torch.cuda.synchronize(dev)
    h = out.cpu().numpy()[:a.n_q * a.n_db * 2].reshape(a.n_db, a.n_q, 2)
    a.close()
    return h[..., 0].copy(), h[..., 1].copy()
