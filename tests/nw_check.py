"""Shared helpers for NW parity tests (imports the oracle: test-only)."""
from __future__ import annotations

import numpy as np

SCHEME = (5, -4, -8, -6)

# (match, mismatch, gap_open, gap_extend) -> the range guard whose edge the
# scheme sits on (DESIGN.md "Scoring-scheme domain")
SCHEMES = {
    (5, -4, -8, -6): "default",
    (2, -3, -5, -2): "small custom scheme",
    (1, 0, 0, 0): "pen = 2, every cell ties",
    (1, 0, -1, 0): "pen = 2, zero extend",
    (5, -4, 0, -6): "zero open: extend ties with open",
    (5, -4, -8, 0): "zero extend: no packed table",
    (8, -8, -16, -12): "pen = 32, rebase refused",
    (12, -4, -20, -16): "pen = 32, larger growth",
    (5, -12, -8, -6): "pen = 34: i32 only",
    (3, -13, -8, -6): "pen = 32, cmm < 0: packed without the table",
    (6, 2, -8, -6): "positive mismatch",
    (-1, -3, -4, -2): "negative match",
    (5, 5, -8, -6): "pen = 0",
    (4, 5, -8, -6): "pen < 0",
    (60, -4, -8, -6): "i32 pen_max = 256",
    (61, -4, -8, -6): "i32 pen_max = 260",
    (5, -4, -8, -20): "steep extend",
    (16, 0, -30, -40): "bonuses near a byte; i32 only (152 columns exceed its int16 range)",
    (5, -4, -6800, -1): "huge open: rebase frame only",
    (5, -4, -2000, -1): "pk_tab_ok accepts",
    (5, -4, -2001, -1): "pk_tab_ok refuses",
    (8, -8, -8, -7): "64-lane rebasing frame near its bound",
    (5, -4, -8, -600): "sentinel reached at 54 columns",
    (5, -4, 2, -6): "positive open",
    (5, -4, -8, 1): "positive extend: i32 only",
    (5, -4, -20, 3): "positive extend: i32 only",
    (5, -4, 2, 1): "positive extend: i32 only (open and extend both positive)",
    (2, -3, 0, 1): "positive extend: i32 only",
    (47, 31, 0, -40): "table bonus byte cm = 254: pk_tab_ok accepts",
    (48, 32, 0, -40): "table bonus byte cm = 256: pk_tab_ok refuses",
    (5, -4, -8, -29): "scale-4 table: 2 cm = 252, accepted",
    (5, -4, -8, -30): "scale-4 table: 2 cm = 260, refused (scale 2)",
    (51, 42, -8, -6): "scale-4 table: 2 cm = 252 from the match, accepted",
    (52, 43, -8, -6): "scale-4 table: 2 cm = 256 from the match, refused",
}
POSITIVE_EXTEND = [(5, -4, -8, 1), (5, -4, 2, 1)]  # the two that every entry point's tests run
SENTINEL_SCHEME = (5, -4, -8, -600)


def rand_seq(rng: np.random.Generator, n: int, alphabet: bytes = b"ACGT") -> bytes:
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def path_score(query: bytes, db: bytes, cigar, scheme=SCHEME) -> tuple[int, bool]:
    """Score of an alignment path under the reference recurrences (I/D open
    only from M, needleman_wunsch_affine.rs:87-94); second value is False if
    the path breaks a recurrence rule or does not consume both sequences."""
    mat, mis, go, ge = scheme
    i = j = 0
    state = "M"
    score = 0
    ok = True
    for n, op in cigar:
        for _ in range(n):
            if op in "=X":
                if j >= len(query) or i >= len(db):
                    return score, False
                eq = query[j] == db[i]
                if (op == "=") != eq:
                    ok = False
                score += mat if eq else mis
                i += 1; j += 1; state = "M"
            elif op == "I":
                if state == "D" or j >= len(query):
                    ok = False
                score += (go + ge) if state == "M" else ge
                j += 1; state = "I"
            else:
                if state == "I" or i >= len(db):
                    ok = False
                score += (go + ge) if state == "M" else ge
                i += 1; state = "D"
    return score, ok and i == len(db) and j == len(query)


def expand(cigar) -> str:
    return "".join(op * n for n, op in cigar)


# ---------------------------------------------- GPU batches against the oracle
PANIC = 2  # SALN_REF_PANIC_BOUNDARY
KINDS = ("iid", "embedded", "disjoint", "prefix", "homopolymer")


def make_pair(rng, kind: str, lq: int, ld: int):
    """iid ACGT; embedded: the shorter side is a window of the longer (the
    largest positive excursion); disjoint: q over {A, C}, d over {G, T} (all
    mismatches, the largest negative one); prefix: the shorter side is the
    longer one's start (the diagonal gains while column 0 drifts);
    homopolymer: a one-letter query; suffix: the shorter side is the longer
    one's end (the diagonal lies in the last rows or columns, where the
    boundary's drift is largest)."""
    if kind == "iid":
        return rand_seq(rng, lq), rand_seq(rng, ld)
    if kind == "disjoint":
        return rand_seq(rng, lq, b"AC"), rand_seq(rng, ld, b"GT")
    if kind == "homopolymer":
        return b"A" * lq, rand_seq(rng, ld)
    long_ = rand_seq(rng, max(lq, ld))
    a = int(rng.integers(0, abs(lq - ld) + 1)) if kind == "embedded" else \
        abs(lq - ld) if kind == "suffix" else 0
    short = long_[a:a + min(lq, ld)]
    return (short, long_) if lq <= ld else (long_, short)


def scheme_seed(scheme) -> int:
    return sum((v & 0xFFFF) << (16 * k) for k, v in enumerate(scheme))


def csr(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    buf = np.frombuffer(b"".join(seqs), np.uint8) if off[-1] else np.zeros(1, np.uint8)
    return np.ascontiguousarray(buf), off


def assert_batch(res, cig_words, want, tag, score_only=False):
    """res: saln_nw_result records; cig_words(k) -> pair k's CIGAR words."""
    bad = np.flatnonzero(res["score"] != want.score)
    assert bad.size == 0, (tag, "score", bad[:8].tolist(), res["score"][bad[:8]].tolist(),
                           want.score[bad[:8]].tolist())
    assert np.array_equal(res["status"] == PANIC, want.panics), (tag, "panic")
    if score_only:
        return
    assert np.array_equal(res["end_states"], want.end_states), (tag, "end states")
    assert np.array_equal(res["printed"].astype(bool), want.cig_len >= 0), (tag, "printed")
    for k in np.flatnonzero(res["printed"]):
        assert np.array_equal(cig_words(int(k)), want.cigar_words(int(k))), (tag, "cigar", int(k))


class PlanRun:
    """One plan over the k-th query against the k-th db, its device buffers,
    and the results of its latest execute."""

    def __init__(self, saln, queries, dbs, scheme, *, full=False, score_only=False, pipelined=False):
        import torch
        self.saln, self.n = saln, len(queries)
        self.qs, self.qo = csr(queries)
        self.ds, self.do = csr(dbs)
        self.plan = saln.NwPlan(self.qo, self.do, pairs=np.stack([np.arange(self.n)] * 2, 1),
                                scoring=scheme, full_codes=full)
        self.score_only, self.pipelined = score_only, pipelined
        if score_only:
            self.plan.set_score_only(True)
        if pipelined:
            self.plan.set_async(True)
        self.dq, self.dd = torch.from_numpy(self.qs.copy()).cuda(), torch.from_numpy(self.ds.copy()).cuda()

    def run(self):
        import torch
        res_t = torch.zeros(self.n * 4, dtype=torch.int32, device="cuda")
        cig_t = None if self.score_only else torch.zeros(max(1, self.plan.cigar_words),
                                                         dtype=torch.int32, device="cuda")
        self.plan.execute(self.dq, self.dd, res_t, cig_t)
        if self.pipelined:
            self.plan.sync()
        torch.cuda.synchronize()
        self.plan.check()
        self.res = res_t.cpu().numpy().view(self.saln._lib.RESULT_DTYPE)
        self.cig = None if cig_t is None else cig_t.cpu().numpy().view(np.uint32)
        return self

    def words(self, k):
        o = int(self.plan.cigar_off[k])
        return self.cig[o:o + int(self.res["cigar_len"][k])]

    def close(self):
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# the launch decisions the guard-edge tests stand on
# decision -> (nw.pk_tab it needs, predicate on a PairPath)
DECISIONS = {
    "single frame": (3, lambda p: p.packed and not p.rebase),
    "rebasing frame": (3, lambda p: p.packed and p.rebase),
    "table scale 2": (1, lambda p: p.table == 2),
    "table scale 4": (2, lambda p: p.table == 4),
    "row profiles": (3, lambda p: p.table == 3),
}
