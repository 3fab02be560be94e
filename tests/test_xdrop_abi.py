"""Host-only ABI of the X-drop extension (include/saln.h,
saln_ends_free_xdrop_*): the refusals, which come before the device is touched,
the unchanged structs, and the Python arguments.  No device: the context
handed in is never read by a call that is refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("saln_ends_free_xdrop_align_batch", "saln_ends_free_sub_xdrop_align_batch",
         "saln_ends_free_xdrop_plan_create", "saln_ends_free_sub_xdrop_plan_create")


class Calls:
    """The four entry points on one pair of len_q x len_db, under the default
    scoring or `matrix`; each returns (status, message)."""

    def __init__(self, saln):
        from sequencealigning_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.ctx_mem = C.create_string_buffer(1 << 14)      # stands for a context; never read
        self.ctx = C.cast(self.ctx_mem, C.c_void_p)

    def _offs(self, n):
        return np.array([0, n], np.uint64)

    def batch(self, len_q, len_db, xdrop, matrix=False, scoring=None):
        qo, do = self._offs(len_q), self._offs(len_db)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = C.c_void_p()
        if matrix is False:
            f, sarg = self.L.saln_ends_free_xdrop_align_batch, self.lib.scoring_arg(scoring)
        else:
            f, sarg = self.L.saln_ends_free_sub_xdrop_align_batch, matrix
        rc = f(self.ctx, None, vp(qo), 1, None, vp(do), 1, None, None, 1, sarg, xdrop, 0, 1, C.byref(out))
        assert not out.value
        return rc, self.lib.last_error()

    def plan(self, len_q, len_db, xdrop, matrix=False, scoring=None):
        qo, do = self._offs(len_q), self._offs(len_db)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = C.c_void_p()
        if matrix is False:
            f, sarg = self.L.saln_ends_free_xdrop_plan_create, self.lib.scoring_arg(scoring)
        else:
            f, sarg = self.L.saln_ends_free_sub_xdrop_plan_create, matrix
        rc = f(self.ctx, vp(qo), 1, vp(do), 1, None, None, 1, sarg, xdrop, C.byref(out))
        assert not out.value
        return rc, self.lib.last_error()


@pytest.fixture(scope="module")
def calls(saln):
    return Calls(saln)


def _matrix(saln):
    return C.pointer(saln.SubstitutionMatrix(b"ACGT", [[5 if a == b else -4 for b in range(4)]
                                                       for a in range(4)], -8, -6).c_struct())


def test_the_header_the_exports_and_the_structs(saln):
    from sequencealigning_amd import _lib
    header = open(os.path.join(ROOT, "include", "saln.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert hasattr(_lib.lib(), name)
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert "int32_t xdrop" in decl and "mode" not in decl
    assert C.sizeof(_lib.EndsFreeResult) == 32 and _lib.EndsFreeResult.reserved.offset == 28
    assert np.dtype(_lib.ENDS_FREE_RESULT_DTYPE).itemsize == 32
    assert C.sizeof(_lib.SubMatrix) == 1292
    assert "X-drop extension" in header and "P < Bin - X" in header


@pytest.mark.parametrize("form", ("batch", "plan"))
def test_a_negative_x_is_refused(saln, calls, form):
    from sequencealigning_amd import _lib
    for x in (-1, -2, -(1 << 31)):
        for matrix in (False, _matrix(saln)):
            rc, msg = getattr(calls, form)(10, 10, x, matrix)
            assert rc == _lib.E_INVALID and "negative" in msg, (x, msg)


@pytest.mark.parametrize("form", ("batch", "plan"))
def test_the_range_guard_counts_x(saln, calls, form):
    """(n + m + 2) max|parameter| + xdrop < 2^30: 22 * 8 = 176 under the default
    scoring."""
    from sequencealigning_amd import _lib
    call = getattr(calls, form)
    for matrix in (False, _matrix(saln)):
        rc, msg = call(10, 10, (1 << 30) - 176, matrix)
        assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, msg
        rc, msg = call(10, 10, (1 << 31) - 1, matrix)
        assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, msg
    # without X the guard is the plain one
    rc, msg = call(1000, 60000, 0, scoring=(1 << 15, -1, -1, -1))
    assert rc == _lib.E_INVALID and "reaches 2^30" in msg and "xdrop" not in msg


@pytest.mark.parametrize("form", ("batch", "plan"))
def test_lengths_over_the_limits_are_refused(saln, calls, form):
    from sequencealigning_amd import _lib
    call = getattr(calls, form)
    for matrix in (False, _matrix(saln)):
        rc, msg = call(1025, 10, 50, matrix)
        assert rc == _lib.E_INVALID and "1025 columns" in msg and "1024" in msg
        rc, msg = call(10, 65001, 50, matrix)
        assert rc == _lib.E_INVALID and "65001 rows" in msg and "65000" in msg


@pytest.mark.parametrize("form", ("batch", "plan"))
def test_a_null_matrix_and_a_scoring_outside_the_domain_are_refused(saln, calls, form):
    from sequencealigning_amd import _lib
    call = getattr(calls, form)
    rc, msg = call(10, 10, 50, matrix=None)
    assert rc == _lib.E_INVALID and "NULL" in msg
    rc, msg = call(10, 10, 50, scoring=(5, 4, -8, -6))
    assert rc == _lib.E_INVALID and "domain" in msg
    assert calls.L.saln_ends_free_xdrop_plan_create(None, None, 0, None, 0, None, None, 0, None, 5, None) \
        == _lib.E_INVALID


def test_python_takes_xdrop_with_extend_only(saln):
    ef = saln.ends_free
    offs = np.array([0, 4], np.uint64)
    for mode in (saln.Mode.Local, saln.Mode.SemiGlobal, ef.OVERLAP):
        with pytest.raises(ValueError, match="EXTEND"):
            ef.ends_free_align_batch([b"ACGT"], [b"ACGT"], mode=mode, xdrop=10)
        with pytest.raises(ValueError, match="EXTEND"):
            ef.EndsFreePlan(offs, offs, mode=mode, xdrop=10)
    with pytest.raises(ValueError, match="integer"):
        ef.ends_free_align_batch([b"ACGT"], [b"ACGT"], mode=ef.EXTEND, xdrop=2.5)
    for long_form in (ef.ends_free_align_long_batch, ef.extend_align_long):
        with pytest.raises(TypeError):
            long_form([b"ACGT"], [b"ACGT"], xdrop=10)
    res = np.zeros(2, dtype=saln._lib.ENDS_FREE_RESULT_DTYPE)
    res["reserved"] = (7, 9)
    assert ef.xdrop_steps(res).tolist() == [7, 9] and saln.xdrop_steps is ef.xdrop_steps
