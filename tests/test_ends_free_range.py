"""The ends-free engine at the accepted edge of its range guard,
(len_q + len_db + 2) * max|parameter| (+ X) < 2^30: the cases that
test_ends_free_range_gpu.py runs, and (here, without a device) the conditions
that keep them honest.  Every value of the engine is a plain int32 with -2^30
as -infinity; the models (ends_free_model.py, xdrop_model.py) compute in int64
with -2^60, so a case whose values come near +-2^30 tells a wrapped, a clamped
or a mistaken -infinity value from a real one.

For a pair of n columns and m rows and an X-drop X, P = (2^30 - 1 - X) //
(n + m + 2) is the largest magnitude the guard accepts.  SCHEMES puts P into
one parameter at a time, into all of them, and into the gaps of a matrix; the
int8 entries of a matrix reach the guard only at n + m + 2 = 2^23, far out of
the plain models' reach, so no case has its largest entry on the edge.

Conditions checked here: every case sits on the edge (one more in P, or in X,
is refused by every entry point family, before the device is touched); the
cases reach both ends of the range (semi-global scores at or below -2^29,
scores of every mode at or above 2^28); the mutated relation's CIGARs hold
'I', 'D' and 'X' in every mode on every path.  They are conditions on the
inputs, not tolerances.

Two of them cannot hold over every listed shape, by arithmetic alone:
  * with m >= n, semi-global of unrelated sequences scores at least -n P (n
    mismatches), which is above -2^29 (n P < 2^30 n / (n + m + 2) <= 2^29); so
    it is asserted for every shape with n > m and n >= 9, which covers every
    lane class and the chunked path.
  * semi-global of an identical prefix d = q[:m] scores (2 m - n - 1) P; among
    the 64-lane shapes only n = m comes near 2^29, so (300, 300) is in CLASS for
    it ((512, 300) gives 0.11 * 2^30).
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import ends_free_model as model
import xdrop_model
from test_extend_gpu import ALPHABET24, TABLE24, anchored, rand_seq

LOCAL, SEMI_GLOBAL, OVERLAP, EXTEND = model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP, model.EXTEND
MODES = (LOCAL, SEMI_GLOBAL, OVERLAP, EXTEND)
LIMIT = 1 << 30

SCALAR = {
    "match": lambda P: (P, -1, 0, -1),
    "mismatch": lambda P: (1, -P, -1, -1),
    "open": lambda P: (5, -4, -P, -1),
    "extend": lambda P: (5, -4, 0, -P),
    "all": lambda P: (P, -P, -P, -P),
    "neg": lambda P: (1, -P, -P, -P),
}
GAPS24 = {"m24_gaps": lambda P: (-P, -P), "m24_ext": lambda P: (0, -P)}
SCHEMES = tuple(SCALAR) + tuple(GAPS24)

TINY = ((1, 1), (1, 5), (2, 1))
# every class with and without pad columns: 16 x 10 (n <= 160), 16 x 16 (<= 256),
# 64 x 8 (<= 512), 64 x 16 (<= 1,024)
CLASS = ((9, 5), (10, 10), (160, 160), (161, 70), (256, 256), (257, 65), (300, 300), (512, 300),
         (513, 64), (1024, 90))
CHUNKED = ((1030, 200), (2100, 130))      # two chunks; three, the third with pad columns
TALL = (70, 65001)                        # a db above the class limit: score only
XDROP_SHAPES = TINY + CLASS             # the class X-drop fill (the tiny pairs: its border product too)
XDROP_LONG = (1030, 70)                 # the chunked X-drop fill
RELATIONS = ("prefix", "mutated", "unrelated")
XKINDS = ("zero", "p", "rest")


def lanes_of(n):
    return 16 if n <= 256 else 64


def edge_p(n, m, X=0):
    return (LIMIT - 1 - X) // (n + m + 2)


def x_case(n, m, xkind):
    """(P, X) of a pair: X = 0; X = P, the fixed point P = (2^30 - 1 - P) //
    (n + m + 2); or a halved P with X the guard's whole remainder."""
    if xkind == "zero":
        return edge_p(n, m), 0
    if xkind == "p":
        P = (LIMIT - 1) // (n + m + 3)
        return P, P
    P2 = edge_p(n, m) // 2
    return P2, LIMIT - 1 - (n + m + 2) * P2


def is_matrix(name):
    return name in GAPS24


@functools.lru_cache(maxsize=None)
def model_scoring(name, P):
    if is_matrix(name):
        return model.matrix_scoring(ALPHABET24, TABLE24, *GAPS24[name](P))
    return model.scalar_scoring(*SCALAR[name](P))


def engine_scoring(saln, name, P):
    if is_matrix(name):
        return saln.SubstitutionMatrix(ALPHABET24, TABLE24, *GAPS24[name](P))
    return SCALAR[name](P)


def max_abs(name, P):
    """The guard's factor of a scheme."""
    if is_matrix(name):
        return max(max(abs(v) for r in TABLE24 for v in r), *(abs(g) for g in GAPS24[name](P)))
    return max(abs(v) for v in SCALAR[name](P))


@functools.lru_cache(maxsize=None)
def relations(n, m, matrix):
    """[(q, d)] in RELATIONS' order: d an identical prefix of q (or q a prefix
    of d), a mutated copy (test_extend_gpu.anchored), and nothing in common (q
    over one half of the letters, d over the other)."""
    letters = ALPHABET24 if matrix else b"ACGT"
    half = len(letters) // 2
    rng = random.Random(0xED6E + 4099 * n + m + (1 << 20) * matrix)
    q = rand_seq(rng, n, letters)
    prefix = q[:m] + rand_seq(rng, max(0, m - n), letters)
    mutated = anchored(rng, q, m, letters)
    return ((q, prefix), (q, mutated), (rand_seq(rng, n, letters[:half]), rand_seq(rng, m, letters[half:])))


_memo = {}


def expect(q, d, mode, name, P):
    """The model's Alignment, once per (q, d, mode, scheme)."""
    key = (q, d, mode, name, P, None)
    if key not in _memo:
        _memo[key] = model.align(q, d, mode, model_scoring(name, P))
    return _memo[key]


def expect_ends(q, d, mode, name, P):
    """(score, q_end, db_end) with rolling rows, for the tall db."""
    key = (q, d, mode, name, P, "ends")
    if key not in _memo:
        _memo[key] = model.linear_ends(q, d, mode, model_scoring(name, P))
    return _memo[key]


def expect_x(q, d, X, name, P):
    """(Alignment, L) of the X-drop model, once per (q, d, scheme, X)."""
    key = (q, d, EXTEND, name, P, X)
    if key not in _memo:
        a, _, L = xdrop_model.align(q, d, X, model_scoring(name, P))
        _memo[key] = (a, L)
    return _memo[key]


# ------------------------------------------------------------------ 1. every case sits on the edge
def test_every_case_sits_on_the_edge():
    for n, m in TINY + CLASS + CHUNKED + (TALL,):
        P = edge_p(n, m)
        assert (n + m + 2) * P < LIMIT <= (n + m + 2) * (P + 1)
        for name in SCHEMES:
            assert max_abs(name, P) == P and max_abs(name, P + 1) == P + 1, (n, m, name)
    assert edge_p(1, 1) == (1 << 28) - 1 and 16 * edge_p(1, 1) >= 1 << 31      # the unread border product
    for n, m in XDROP_SHAPES + (XDROP_LONG,):
        for xkind in XKINDS:
            P, X = x_case(n, m, xkind)
            assert (n + m + 2) * P + X < LIMIT <= (n + m + 2) * (P + 1) + X, (n, m, xkind)
            assert 0 <= X < 1 << 31 and P > max(abs(v) for r in TABLE24 for v in r)
        P, X = x_case(n, m, "rest")
        assert (n + m + 2) * P + X == LIMIT - 1 and X >= 1 << 29              # X + 1 is refused
        assert x_case(n, m, "p")[1] == x_case(n, m, "p")[0]


class Calls:
    """The entry point families on one pair of n x m, each returning (status,
    message).  The refusals come before the device is touched: the context
    handed in is a zeroed block, which reads as a context without option
    overrides (the replay entry point looks up its tile rows first)."""

    BATCH = {"class": "saln_ends_free_%salign_batch", "long": "saln_ends_free_%slong_align_batch",
             "replay": "saln_ends_free_%sreplay_align_batch"}
    XBATCH = {"xdrop": "saln_ends_free_%sxdrop_align_batch", "xdrop_long": "saln_ends_free_%sxdrop_long_align_batch"}
    FAMILIES = ("class", "plan", "long", "replay", "xdrop", "xdrop_plan", "xdrop_long")

    def __init__(self, saln):
        from sequencealigning_amd import _lib
        self.saln, self.lib, self.L = saln, _lib, _lib.lib()
        self.ctx_mem = C.create_string_buffer(1 << 14)
        self.ctx = C.cast(self.ctx_mem, C.c_void_p)

    def sarg(self, name, P):
        """(the scoring argument, the infix of the entry points that take it)."""
        if is_matrix(name):
            return C.pointer(engine_scoring(self.saln, name, P).c_struct()), "sub_"
        return self.lib.scoring_arg(SCALAR[name](P)), ""

    def call(self, family, n, m, sarg, infix, mode=EXTEND, xdrop=0):
        qo, do = np.array([0, n], np.uint64), np.array([0, m], np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = C.c_void_p()
        if family in self.BATCH:
            rc = getattr(self.L, self.BATCH[family] % infix)(
                self.ctx, None, vp(qo), 1, None, vp(do), 1, None, None, 1, mode, sarg, 0, 1, C.byref(out))
        elif family in self.XBATCH:
            rc = getattr(self.L, self.XBATCH[family] % infix)(
                self.ctx, None, vp(qo), 1, None, vp(do), 1, None, None, 1, sarg, xdrop, 0, 1, C.byref(out))
        elif family == "plan":
            rc = getattr(self.L, "saln_ends_free_%splan_create" % infix)(
                self.ctx, vp(qo), 1, vp(do), 1, None, None, 1, mode, sarg, C.byref(out))
        else:
            rc = getattr(self.L, "saln_ends_free_%sxdrop_plan_create" % infix)(
                self.ctx, vp(qo), 1, vp(do), 1, None, None, 1, sarg, xdrop, C.byref(out))
        assert not out.value
        return rc, self.lib.last_error()


@pytest.fixture(scope="module")
def calls(saln):
    return Calls(saln)


@pytest.mark.parametrize("family", Calls.FAMILIES)
def test_one_more_is_refused(saln, calls, family):
    """P + 1 in the place of P, under an X-drop at the case's X; and at the
    case's P the first X the guard refuses: X + 1 where X is the guard's
    remainder, at most n + m + 2 above X where X = P."""
    from sequencealigning_amd import _lib
    any_length = family in ("long", "replay", "xdrop_long")
    xdrop = family.startswith("xdrop")
    shapes = XDROP_SHAPES + (XDROP_LONG,) if family == "xdrop_long" else XDROP_SHAPES if xdrop else \
        TINY + CLASS + (CHUNKED + (TALL,) if any_length else ())
    refused = 0
    for n, m in shapes:
        for name in SCHEMES:
            if not xdrop:
                sarg, infix = calls.sarg(name, edge_p(n, m) + 1)
                for mode in MODES:
                    rc, msg = calls.call(family, n, m, sarg, infix, mode)
                    assert rc == _lib.E_INVALID and "2^30" in msg and "xdrop" not in msg, (n, m, name, mode, msg)
                    refused += 1
                continue
            for xkind in XKINDS:
                P, X = x_case(n, m, xkind)
                sarg, infix = calls.sarg(name, P + 1)
                rc, msg = calls.call(family, n, m, sarg, infix, xdrop=X)
                assert rc == _lib.E_INVALID and "2^30" in msg, (n, m, name, xkind, msg)
                refused += 1
                if xkind != "zero":
                    # at this P the first refused X: X + 1 for the remainder, within n + m + 2 of X = P
                    first = LIMIT - (n + m + 2) * P
                    assert first == X + 1 if xkind == "rest" else X < first <= X + n + m + 2
                    sarg, infix = calls.sarg(name, P)
                    rc, msg = calls.call(family, n, m, sarg, infix, xdrop=first)
                    assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, (n, m, name, msg)
                    refused += 1
    assert refused >= len(shapes) * len(SCHEMES) * 4


# ------------------------------------------------------------------ 2. both ends of the range
def test_semi_global_reaches_the_negative_end():
    """`neg`, nothing in common: at or below -2^29 at every shape with n > m
    (the module's text has why not at the others), in every lane class and on
    the chunked path."""
    seen = set()
    for n, m in CLASS + CHUNKED:
        if n < 9 or n <= m:
            continue
        P = edge_p(n, m)
        q, d = relations(n, m, False)[2]
        a = expect(q, d, SEMI_GLOBAL, "neg", P)
        assert -LIMIT < a.score <= -(1 << 29), (n, m, a.score / LIMIT)
        seen.add("chunked" if n > 1024 else model_class(n))
    assert seen == {(16, 10), (16, 16), (64, 8), (64, 16), "chunked"}
    q, d = relations(2100, 130, False)[2]
    assert expect(q, d, SEMI_GLOBAL, "neg", edge_p(2100, 130)).score < -0.93 * LIMIT


def model_class(n):
    return next((g, k) for g, k in ((16, 10), (16, 16), (64, 8), (64, 16)) if n <= g * k)


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_reaches_the_positive_end(mode):
    """`all`, d an identical prefix: a score of at least 2^28 among the shapes
    of 16 lanes and among those of 64."""
    for lanes in (16, 64):
        scores = {}
        for n, m in CLASS:
            if lanes_of(n) == lanes:
                q, d = relations(n, m, False)[0]
                scores[n, m] = expect(q, d, mode, "all", edge_p(n, m)).score
        assert max(scores.values()) >= 1 << 28, (lanes, {k: v / LIMIT for k, v in scores.items()})
        assert all(v < LIMIT for v in scores.values())
    q, d = relations(9, 5, False)[0]
    if mode != SEMI_GLOBAL:
        assert expect(q, d, mode, "all", edge_p(9, 5)).score == 5 * edge_p(9, 5) > 0.31 * LIMIT


# ------------------------------------------------------------------ 3. the CIGARs are not trivial
@pytest.mark.parametrize("path", ("class", "chunked"))
@pytest.mark.parametrize("mode", MODES)
def test_mutated_cigars_hold_every_op(mode, path):
    """Per mode and path (the replay walks the chunked path's shapes) a mutated
    case whose CIGAR holds 'I', 'D' and 'X'."""
    shapes = CHUNKED if path == "chunked" else tuple(reversed(CLASS))
    cases = ((n, m, name) for name in ("all",) + SCHEMES for n, m in shapes)
    for n, m, name in cases:
        q, d = relations(n, m, is_matrix(name))[1]
        if {"I", "D", "X"} <= {op for _, op in expect(q, d, mode, name, edge_p(n, m)).cigar}:
            return
    raise AssertionError((mode, path))
