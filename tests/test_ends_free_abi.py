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


def test_cigar_score():
    from sequencealigning_amd.ends_free import cigar_score
    assert cigar_score([(4, "="), (1, "X"), (2, "I"), (3, "=")]) == 20 - 4 - 8 - 12 + 15
    assert cigar_score([(2, "D"), (1, "=")], (1, -1, 0, -1)) == -2 + 1
