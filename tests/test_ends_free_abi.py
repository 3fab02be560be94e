"""Host-only ABI of the ends-free engine (include/saln.h, saln_ends_free_*):
the record's size, the code size of a pair and the query classes.  No device."""
import ctypes

import numpy as np
import pytest


def test_result_is_32_bytes(saln):
    from sequencealigning_amd import _lib
    assert ctypes.sizeof(_lib.EndsFreeResult) == 32
    assert np.dtype(_lib.ENDS_FREE_RESULT_DTYPE).itemsize == 32
    names = [f[0] for f in _lib.EndsFreeResult._fields_]
    assert names == [f[0] for f in _lib.ENDS_FREE_RESULT_DTYPE] == [
        "score", "status", "q_begin", "q_end", "db_begin", "db_end", "cigar_len", "reserved"]


def test_trace_bytes_is_monotone_and_zero_for_an_empty_side(saln):
    ef = saln.ends_free
    for n in (0, 1, 5, 1024):
        assert ef.trace_bytes(n, 0) == 0
        assert ef.trace_bytes(0, n) == 0
    for m in (1, 2, 63, 300):
        prev = 0
        for n in range(1, 1025):
            b = ef.trace_bytes(n, m)
            assert b >= prev and b >= (n * m + 1) // 2, (n, m)   # 4 bits per cell at least
            lanes, cols = ef.pair_geometry(n)
            assert b <= m * ((n + cols - 1) // cols * cols // 2) + 8, (n, m)  # whole lanes, no more
            prev = b
    for n in (1, 150, 161, 1024):
        prev = 0
        for m in range(1, 200):
            b = ef.trace_bytes(n, m)
            assert b >= prev
            prev = b


def test_pair_geometry_covers_every_query(saln):
    ef = saln.ends_free
    classes = []
    for n in range(1, 1025):
        lanes, cols = ef.pair_geometry(n)
        assert lanes in (16, 64) and cols % 2 == 0
        assert lanes * cols >= n
        if (lanes, cols) not in classes:
            classes.append((lanes, cols))
    # the classes grow with the query: every cap is the last length of its class
    caps = [lanes * cols for lanes, cols in classes]
    assert caps == sorted(caps) and caps[-1] == 1024
    for c in caps[:-1]:
        assert ef.pair_geometry(c) != ef.pair_geometry(c + 1)


def test_limits_are_refused_with_a_message(saln):
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    with pytest.raises(_lib.SalnError) as e:
        ef.pair_geometry(1025)
    assert e.value.code == _lib.E_INVALID and "1024" in str(e.value)
    with pytest.raises(_lib.SalnError) as e:
        ef.trace_bytes(1025, 10)
    assert e.value.code == _lib.E_INVALID and "1024" in str(e.value)


def test_fill_geometry_is_the_staging_formula(saln):
    """saln_ends_free_fill_geometry: 256 / lanes groups, lowered until groups *
    (ld_max + 2 lanes) fits 64 KB (less the matrix's 1,408 bytes), never below 1."""
    import os
    import re
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "saln.h")).read()
    assert "saln_ends_free_fill_geometry" in _lib.EXPORTS
    assert re.search(r"\bint saln_ends_free_fill_geometry\(uint64_t len_q, uint64_t ld_max, int has_matrix, "
                     r"uint32_t \*groups,\s+uint32_t \*lds_bytes\);", header)
    for n in (0, 1, 160, 161, 256, 257, 512, 513, 1024):
        lanes = ef.pair_geometry(n)[0] if n else 16
        for matrix in (False, True):
            budget = (64 << 10) - (1408 if matrix else 0)
            for ld in (0, 1, 400, 3976, 3977, 4000, 4064, 4065, 16256, 16257, 31936, 31937, 32736, 32737, 65000):
                groups, lds = ef.fill_geometry(n, ld, matrix)
                want = max(1, min(256 // lanes, budget // (ld + 2 * lanes)))
                assert (groups, lds) == (want, want * (ld + 2 * lanes)), (n, ld, matrix)
                assert lds <= budget or groups == 1
    assert ef.fill_geometry(100, 4000) == (16, 64512) and ef.fill_geometry(100, 4000, True) == (15, 60480)


def test_fill_geometry_refusals(saln):
    from sequencealigning_amd import _lib
    ef, L = saln.ends_free, _lib.lib()
    g, b = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert L.saln_ends_free_fill_geometry(10, 10, 0, None, ctypes.byref(b)) == _lib.E_INVALID
    assert L.saln_ends_free_fill_geometry(10, 10, 0, ctypes.byref(g), None) == _lib.E_INVALID
    assert (g.value, b.value) == (7, 7)
    with pytest.raises(_lib.SalnError) as e:
        ef.fill_geometry(1025, 10)
    assert e.value.code == _lib.E_INVALID and "1024" in str(e.value)
    with pytest.raises(_lib.SalnError) as e:
        ef.fill_geometry(10, 65001, True)
    assert e.value.code == _lib.E_INVALID and "65000" in str(e.value)
    assert L.saln_ends_free_fill_geometry(1025, 10, 0, ctypes.byref(g), ctypes.byref(b)) == _lib.E_INVALID
    assert (g.value, b.value) == (7, 7)                    # a refused call writes nothing
    assert ef.fill_geometry(1024, 65000) == (1, 65128)


def test_cigar_score():
    from sequencealigning_amd.ends_free import cigar_score
    assert cigar_score([(4, "="), (1, "X"), (2, "I"), (3, "=")]) == 20 - 4 - 8 - 12 + 15
    assert cigar_score([(2, "D"), (1, "=")], (1, -1, 0, -1)) == -2 + 1
