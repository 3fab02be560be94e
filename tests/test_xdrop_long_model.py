"""Holds tests/xdrop_long_model.py, the chunked X-drop fill's schedule (row
windows per chunk, dead chunks, the pair's stop; saln_ends_free_xdrop_long_*),
to the plain xdrop_model at chunk widths 2, 4 and 8, where small pairs meet
every rule; then the step bound, the host-only refusals of the two new entry
points and the Python arguments.  CPU only: a refused call never reads the
context it is handed."""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest

import ends_free_model as efm
import xdrop_long_model as lm
import xdrop_model as model
from test_extend_gpu import anchored, rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (5, -4, -8, -6)
OPEN0 = (5, -4, 0, -3)
WIDTHS = (2, 4, 8)
NAMES = ("saln_ends_free_xdrop_long_align_batch", "saln_ends_free_sub_xdrop_long_align_batch")
# a small asymmetric matrix over four symbols
ASYM = [[6, -3, -5, -2], [-4, 7, -1, -6], [-5, -2, 5, -3], [-1, -6, -4, 8]]


def scorings():
    return [efm.scalar_scoring(*DEFAULT), efm.scalar_scoring(*OPEN0),
            efm.matrix_scoring(b"ACGT", ASYM, -5, -2)]


def trap_b_rows(rows, alive, n, m, W):
    """Rows i and boundary columns c0 = k W where (i, c0) is pruned, its B lies
    above B(i - 1, c0), and the next chunk holds an unpruned cell in row i: a
    chunk that took B(i, c0) from the row above would prune by another B."""
    count = 0
    for c0 in range(W, n, W):
        for i in range(1, m + 1):
            if not alive[i, c0] and rows[i][c0][3] > rows[i - 1][c0][3] \
                    and alive[i, c0 + 1:min(n, c0 + W) + 1].any():
                count += 1
    return count


def check_pair(q, d, X, sc, W):
    """The schedule against the plain model; returns the pair's trap-(b) rows."""
    want, alive, L = model.align(q, d, X, sc, stop=False)
    rows = model.fill(q, d, X, sc, stop=False)
    got, galive, computed, windows, steps = lm.align(q, d, X, sc, W)
    assert got == want, (q, d, X, W)
    assert (galive == (alive & computed)).all(), (q, d, X, W)
    assert not alive[~computed].any(), (q, d, X, W)          # every skipped cell is pruned
    cells = lm.schedule(q, d, X, sc, W)[0]
    for (i, j), cell in cells.items():
        assert cell == rows[i][j], (q, d, X, W, i, j)         # B included
    n, m = len(q), len(d)
    assert len(windows) <= (n + W - 1) // W and all(1 <= a <= z <= m for a, z in windows)
    assert all(a0 <= a1 and z0 <= z1 for (a0, z0), (a1, z1) in zip(windows, windows[1:]))
    assert steps == lm.steps_bound(windows)
    assert lm.align(q, d, X, sc, W, walk=False)[0] == model.align(q, d, X, sc, walk=False)[0]
    return trap_b_rows(rows, alive, n, m, W)


@pytest.mark.parametrize("W", WIDTHS)
def test_every_small_pair(W):
    sc = efm.scalar_scoring(*DEFAULT)
    seqs = [bytes(s) for k in range(6) for s in itertools.product(b"AC", repeat=k)]
    for q in seqs:
        for d in seqs:
            for X in (0, 1, 3, model.no_drop(len(q), len(d), sc)):
                check_pair(q, d, X, sc, W)


@pytest.mark.parametrize("W", WIDTHS)
def test_random_pairs_meet_trap_b(W):
    """About 1,000 pairs per width under three scorings; the set must hold rows
    of trap (b), or it could pass without ever meeting it."""
    rng = random.Random(0x10C9 + W)
    traps = windows_cut = stopped = 0
    for k in range(1000):
        sc = scorings()[k % 3]
        q = rand_seq(rng, rng.randint(0, 40), b"ACGT")
        d = anchored(rng, q, rng.randint(0, 40), b"ACGT")
        X = rng.choice((0, 5, 9, 14, 20, 30, 45, 80, 10 ** 6))
        traps += check_pair(q, d, X, sc, W)
        w = lm.schedule(q, d, X, sc, W)[2]
        windows_cut += sum(a > 1 for a, _ in w)
        stopped += len(w) < (len(q) + W - 1) // W and len(d) > 0
    assert traps > 0, "no row of trap (b) in the set"
    assert windows_cut > 50 and stopped > 50                  # chunks starting below row 1; pairs ending early


def test_a_stale_boundary_entry_is_poison():
    """Trap (a): the slot raises on a row the chunk before did not publish."""
    slot = lm._Slot({3: (1, 2, 3)})
    assert slot[3] == (1, 2, 3)
    with pytest.raises(AssertionError, match="did not publish"):
        slot[4]


def test_the_step_bound():
    """Per chunk run: its rows, 63 steps of skew, one for the vote; no term for
    the refill period.  The kernel's chunk width, on a diagonal pair: chunk 1
    starts far below row 1, and the bound lies far below the plain fill's
    2 x (1,100 + 63)."""
    assert lm.steps_bound([]) == 0
    assert lm.steps_bound([(1, 1)]) == 65 and lm.steps_bound([(1, 100), (90, 130)]) == 164 + 105
    assert lm.steps_bound([(5, 9)], lanes=16) == 21
    rng = random.Random(0xD1A6)
    q = rand_seq(rng, 1100, b"ACGT")
    d = bytearray(q)
    for k in range(8, 1092):
        if rng.random() < 0.05:
            d[k] = rng.choice(b"ACGT")
    windows = lm.schedule(q, bytes(d), 60)[2]
    assert len(windows) == 2 and windows[0][0] == 1 and windows[1][0] > 1000
    assert lm.steps_bound(windows) < 2 * (1100 + 63) * 0.7


# ---------------------------------------------------------------- the ABI, host only
class Calls:
    def __init__(self):
        from sequencealigning_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.ctx_mem = C.create_string_buffer(1 << 14)      # stands for a context; never read
        self.ctx = C.cast(self.ctx_mem, C.c_void_p)

    def batch(self, len_q, len_db, xdrop, matrix=False, scoring=None):
        qo, do = np.array([0, len_q], np.uint64), np.array([0, len_db], np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = C.c_void_p()
        if matrix is False:
            f, sarg = self.L.saln_ends_free_xdrop_long_align_batch, self.lib.scoring_arg(scoring)
        else:
            f, sarg = self.L.saln_ends_free_sub_xdrop_long_align_batch, matrix
        rc = f(self.ctx, None, vp(qo), 1, None, vp(do), 1, None, None, 1, sarg, xdrop, 0, 1, C.byref(out))
        assert not out.value
        return rc, self.lib.last_error()


@pytest.fixture(scope="module")
def calls(saln):
    return Calls()


def _matrix(saln):
    return C.pointer(saln.SubstitutionMatrix(b"ACGT", ASYM, -5, -2).c_struct())


def test_the_header_and_the_exports(saln):
    from sequencealigning_amd import _lib
    header = open(os.path.join(ROOT, "include", "saln.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert "int32_t xdrop" in decl and "mode" not in decl
    flat = re.sub(r"[\s*]+", " ", header)
    assert "The chunked fill and the tiled replay have no X-drop form" not in flat
    assert saln.xdrop_extend_long_batch is saln.ends_free.xdrop_extend_long_batch
    assert saln.xdrop_extend_long is saln.ends_free.xdrop_extend_long


def test_a_negative_x_is_refused(saln, calls):
    from sequencealigning_amd import _lib
    for x in (-1, -2, -(1 << 31)):
        for matrix in (False, _matrix(saln)):
            rc, msg = calls.batch(3000, 70000, x, matrix)
            assert rc == _lib.E_INVALID and "negative" in msg, (x, msg)


def test_the_range_guard_counts_x_and_is_the_only_limit(saln, calls):
    """(n + m + 2) max|parameter| + xdrop < 2^30: (3,000 + 70,000 + 2) * 8 =
    584,016 under both scorings here (the matrix's largest magnitude is 8)."""
    from sequencealigning_amd import _lib
    for matrix in (False, _matrix(saln)):
        rc, msg = calls.batch(3000, 70000, (1 << 30) - 584016, matrix)
        assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, msg
        rc, msg = calls.batch(10, 10, (1 << 31) - 1, matrix)
        assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, msg
    rc, msg = calls.batch(1 << 27, 10, 0)
    assert rc == _lib.E_INVALID and "reaches 2^30" in msg and "columns" not in msg


def test_a_null_matrix_and_a_scoring_outside_the_domain_are_refused(saln, calls):
    from sequencealigning_amd import _lib
    rc, msg = calls.batch(3000, 10, 50, matrix=None)
    assert rc == _lib.E_INVALID and "NULL" in msg
    rc, msg = calls.batch(3000, 10, 50, scoring=(5, 4, -8, -6))
    assert rc == _lib.E_INVALID and "domain" in msg


def test_python_refuses_a_non_integer_xdrop(saln):
    ef = saln.ends_free
    for x in (2.5, True, None, "7"):
        with pytest.raises((ValueError, TypeError), match="integer"):
            ef.xdrop_extend_long_batch([b"ACGT"], [b"ACGT"], xdrop=x)
        with pytest.raises((ValueError, TypeError), match="integer"):
            ef.xdrop_extend_long(b"ACGT", b"ACGT", xdrop=x)
    with pytest.raises(TypeError):
        ef.xdrop_extend_long_batch([b"ACGT"], [b"ACGT"])          # xdrop is required
    with pytest.raises(ValueError, match="direction"):
        ef.xdrop_extend_long(b"ACGT", b"ACGT", xdrop=5, direction="up")
