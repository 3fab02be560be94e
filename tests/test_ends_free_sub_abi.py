"""Host-only ABI of the ends-free engine under a substitution matrix
(include/saln.h, saln_sub_matrix and saln_sub_matrix_check) and its Python
face (SubstitutionMatrix, from_ncbi, alignment_score).  No device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(saln, n_sym=3, gap_open=-3, gap_extend=-1, fill=-2, diag=4):
    """A valid saln_sub_matrix: every byte maps to byte % n_sym."""
    from sequencealigning_amd import _lib
    m = _lib.SubMatrix()
    m.n_sym = n_sym
    m.gap_open, m.gap_extend = gap_open, gap_extend
    for b in range(256):
        m.code[b] = b % n_sym if n_sym else 0
    for a in range(32):
        for b in range(32):
            m.score[a][b] = diag if a == b else fill
    return m


def _check(saln, m):
    from sequencealigning_amd import _lib
    mx = ctypes.c_int32(-1)
    rc = _lib.lib().saln_sub_matrix_check(ctypes.byref(m), ctypes.byref(mx))
    return rc, mx.value, _lib.last_error()


def test_struct_matches_the_header(saln):
    from sequencealigning_amd import _lib
    assert ctypes.sizeof(_lib.SubMatrix) == 4 + 8 + 256 + 32 * 32 == 1292
    assert _lib.SubMatrix.gap_open.offset == 4 and _lib.SubMatrix.code.offset == 12
    assert _lib.SubMatrix.score.offset == 268
    header = open(os.path.join(ROOT, "include", "saln.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} saln_sub_matrix;", header).group(1)
    fields = re.findall(r"(\w+)(?:\[\d+\])*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in _lib.SubMatrix._fields_]
    for name in ("saln_sub_matrix_check", "saln_ends_free_sub_align_batch",
                 "saln_ends_free_sub_long_align_batch", "saln_ends_free_sub_replay_align_batch",
                 "saln_ends_free_sub_plan_create"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\(" % name, header), name
        assert hasattr(_lib.lib(), name)


def test_check_accepts_and_reports_the_largest_magnitude(saln):
    from sequencealigning_amd import _lib
    assert _check(saln, _matrix(saln))[:2] == (_lib.OK, 4)
    assert _check(saln, _matrix(saln, n_sym=1))[:2] == (_lib.OK, 4)
    assert _check(saln, _matrix(saln, n_sym=32, gap_open=0, gap_extend=-9))[:2] == (_lib.OK, 9)
    m = _matrix(saln)
    m.score[2][0] = -128                       # inside n_sym x n_sym: counts
    assert _check(saln, m)[:2] == (_lib.OK, 128)
    m = _matrix(saln)
    m.score[3][0] = -128                       # at or above n_sym: ignored
    m.score[0][31] = 127
    assert _check(saln, m)[:2] == (_lib.OK, 4)
    assert _lib.lib().saln_sub_matrix_check(ctypes.byref(_matrix(saln)), None) == _lib.OK


@pytest.mark.parametrize("what, edit, word", [
    ("n_sym 0", lambda m: setattr(m, "n_sym", 0), "n_sym"),
    ("n_sym 33", lambda m: setattr(m, "n_sym", 33), "n_sym"),
    ("a code at n_sym", lambda m: m.code.__setitem__(200, 3), "code[200]"),
    ("gap_extend 0", lambda m: setattr(m, "gap_extend", 0), "gap_extend"),
    ("gap_extend > 0", lambda m: setattr(m, "gap_extend", 1), "gap_extend"),
    ("gap_open > 0", lambda m: setattr(m, "gap_open", 1), "gap_open"),
    ("reserved", lambda m: m.reserved.__setitem__(1, 1), "reserved"),
])
def test_check_refuses(saln, what, edit, word):
    from sequencealigning_amd import _lib
    m = _matrix(saln)
    edit(m)
    rc, _, msg = _check(saln, m)
    assert rc == _lib.E_INVALID, what
    assert word in msg, (what, msg)


def test_check_refuses_a_matrix_without_a_positive_entry(saln):
    from sequencealigning_amd import _lib
    m = _matrix(saln, diag=0)
    m.score[0][3] = 5                          # outside n_sym x n_sym: does not count
    m.score[31][31] = 5
    rc, _, msg = _check(saln, m)
    assert rc == _lib.E_INVALID and "> 0" in msg
    m.score[2][1] = 1                          # one off-diagonal entry is enough
    assert _check(saln, m)[0] == _lib.OK
    assert _lib.lib().saln_sub_matrix_check(None, None) == _lib.E_INVALID


# ------------------------------------------------------------------ SubstitutionMatrix
TABLE3 = [[4, -3, 2], [-2, 3, 0], [-4, -5, -1]]


def test_substitution_matrix_maps_and_orients(saln):
    sm = saln.SubstitutionMatrix(b"ACG", TABLE3, -3, -1)
    assert sm.n_sym == 4 and sm.unknown == -5
    assert sm.s(ord("A"), ord("G")) == 2 and sm.s(ord("G"), ord("A")) == -4   # s(db, query)
    assert sm.s(ord("T"), ord("A")) == -5 and sm.s(ord("A"), ord("T")) == -5 and sm.s(0, 255) == -5
    assert sm.s(ord("a"), ord("A")) == -5                                     # case matters by default
    c = sm.c_struct()
    assert c.n_sym == 4 and (c.gap_open, c.gap_extend) == (-3, -1) and list(c.reserved) == [0, 0, 0]
    assert [c.code[b] for b in b"ACGTN"] == [0, 1, 2, 3, 3] and all(v < 4 for v in c.code)
    assert [[c.score[a][b] for b in range(4)] for a in range(4)] == [
        [4, -3, 2, -5], [-2, 3, 0, -5], [-4, -5, -1, -5], [-5, -5, -5, -5]]
    assert sm.check() == 5
    assert saln.SubstitutionMatrix(b"ACG", TABLE3, -3, -1, unknown=-9).check() == 9
    assert saln.SubstitutionMatrix(b"ACG", TABLE3, -3, -1, unknown=1).s(ord("T"), ord("T")) == 1


def test_substitution_matrix_case_insensitive(saln):
    sm = saln.SubstitutionMatrix(b"AcG", TABLE3, -3, -1, case_insensitive=True)
    assert sm.s(ord("a"), ord("g")) == 2 and sm.s(ord("C"), ord("c")) == 3
    assert sm.s(ord("t"), ord("a")) == -5
    with pytest.raises(ValueError, match="duplicate"):
        saln.SubstitutionMatrix(b"Aa", [[1, 0], [0, 1]], -1, -1, case_insensitive=True)
    saln.SubstitutionMatrix(b"Aa", [[1, 0], [0, 1]], -1, -1)   # two symbols when case matters


def test_substitution_matrix_value_errors(saln):
    SM = saln.SubstitutionMatrix
    with pytest.raises(ValueError, match="duplicate"):
        SM(b"ACA", TABLE3, -3, -1)
    with pytest.raises(ValueError, match="int8"):
        SM(b"AC", [[1, 128], [0, 1]], -3, -1)
    with pytest.raises(ValueError, match="int8"):
        SM(b"AC", [[1, -129], [0, 1]], -3, -1)
    with pytest.raises(ValueError, match="int8"):
        SM(b"AC", [[1, 0], [0, 1]], -3, -1, unknown=-200)
    with pytest.raises(ValueError, match="2 x 2"):
        SM(b"AC", [[1, 0, 0], [0, 1, 0]], -3, -1)
    with pytest.raises(ValueError, match="2 x 2"):
        SM(b"AC", [[1, 0]], -3, -1)
    big = bytes(range(65, 65 + 32))
    with pytest.raises(ValueError, match="at most 31"):
        SM(big, [[1] * 32] * 32, -3, -1)
    ok = SM(big[:31], [[1] * 31] * 31, -3, -1)
    assert ok.n_sym == 32 and ok.check() == 3
    with pytest.raises(ValueError):
        SM(b"", [], -3, -1)


def test_domain_errors_come_from_the_library(saln):
    from sequencealigning_amd import _lib
    for args in ((b"AC", [[1, 0], [0, 1]], 1, -1), (b"AC", [[1, 0], [0, 1]], 0, 0),
                 (b"AC", [[0, -1], [-1, 0]], -1, -1)):
        with pytest.raises(_lib.SalnError) as e:
            saln.SubstitutionMatrix(*args).check()
        assert e.value.code == _lib.E_INVALID


NCBI = """\
# a small matrix in the usual text form
#  rows: the db symbol
   A  C  G  *
A  4 -3  2 -6   # trailing comment
C -2  3  0 -6
G -4 -5 -1 -6

*  -6 -6 -6 1
"""


def test_from_ncbi(saln):
    sm = saln.SubstitutionMatrix.from_ncbi(NCBI, -3, -1)
    assert sm.alphabet == b"ACG" and sm.unknown == 1 and (sm.gap_open, sm.gap_extend) == (-3, -1)
    assert [[sm.s(a, b) for b in b"ACG"] for a in b"ACG"] == TABLE3
    assert sm.s(ord("T"), ord("A")) == 1
    sm = saln.SubstitutionMatrix.from_ncbi(NCBI.encode(), -3, -1, unknown=-8, case_insensitive=True)
    assert sm.unknown == -8 and sm.s(ord("a"), ord("g")) == 2
    plain = "A C\nA 1 -1\nC -2 1\n"
    sm = saln.SubstitutionMatrix.from_ncbi(plain, 0, -1)
    assert sm.alphabet == b"AC" and sm.unknown == -2 and sm.s(ord("C"), ord("A")) == -2
    for bad in ("", "A C\nA 1 -1\n", "A C\nA 1 -1\nG -2 1\n", "A C\nA 1\nC -2 1\n",
                "A C\nA 1 x\nC -2 1\n", "AB C\nAB 1 1\nC 1 1\n"):
        with pytest.raises(ValueError):
            saln.SubstitutionMatrix.from_ncbi(bad, 0, -1)


def test_alignment_score(saln):
    from sequencealigning_amd.ends_free import alignment_score, cigar_score
    sm = saln.SubstitutionMatrix(b"ACG", TABLE3, -3, -1)
    q, d = b"TTGACGA", b"AACCG"
    # query G on db A (2), A on A (4), then 'C' inserted, then G on C (0), A on C (-2)
    cigar = [(1, "X"), (1, "="), (1, "I"), (2, "X")]
    assert alignment_score(q, d, cigar, sm, 2, 0) == 2 + 4 + (-3 - 1) + 0 - 2
    assert alignment_score(q, d, [(2, "D"), (1, "X")], sm, 2, 0) == -3 - 2 + sm.s(ord("C"), ord("G"))
    scalar = (5, -4, -8, -6)
    assert alignment_score(q, d, cigar, scalar, 2, 0) == cigar_score(cigar, scalar)
    assert alignment_score(q, d, cigar, None, 2, 0) == cigar_score(cigar)
    with pytest.raises(ValueError):
        alignment_score(q, d, [(1, "=")], sm, 2, 0)        # the bytes differ
    with pytest.raises(ValueError):
        alignment_score(q, d, [(9, "I")], sm, 2, 0)        # past the query's end
    import numpy as np
    from sequencealigning_amd import _lib
    rec = np.zeros(1, dtype=_lib.ENDS_FREE_RESULT_DTYPE)[0]
    rec["q_begin"], rec["db_begin"] = 2, 0
    assert alignment_score(q, d, (rec, cigar), sm) == 0
