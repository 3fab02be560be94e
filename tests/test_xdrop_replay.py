"""CPU, no device: the host-only side of the X-drop extension's tiled replay
(saln_ends_free_xdrop_replay_align_batch, its matrix form and
saln_ends_free_xdrop_replay_bytes): the exports and the
header, the footprint against its stated formula and three pinned values, the
refusals, which all happen before the device is touched (a refused call never
reads the context it is handed beyond its options), and the Python argument."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_xdrop_long_model import ASYM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("saln_ends_free_xdrop_replay_align_batch", "saln_ends_free_sub_xdrop_replay_align_batch")
TILE_ROWS = (64, 128, 256, 512, 1024)
CHUNK = 1024


def footprint(n, m, R):
    """The stated formula of a chunked-path pair: a header per chunk, the kept
    boundary columns, the checkpoint rows, the tile in work."""
    chunks = (n + CHUNK - 1) // CHUNK
    return chunks * 16 + (chunks - 1) * m * 16 + (m - 1) // R * chunks * CHUNK * 16 + R * 512


def test_the_header_and_the_exports(saln):
    from sequencealigning_amd import _lib
    header = open(os.path.join(ROOT, "include", "saln.h")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert "int32_t xdrop" in decl and "mode" not in decl
    name = "saln_ends_free_xdrop_replay_bytes"
    assert name in _lib.EXPORTS and hasattr(_lib.lib(), name) and re.search(r"\b%s\(" % name, header)
    flat = re.sub(r"[\s*]+", " ", header)
    assert "The tiled replay has no X-drop form" not in flat
    assert "replay has no X-drop" not in flat
    assert callable(saln.ends_free.xdrop_replay_bytes)


def test_the_three_pins(saln):
    ef = saln.ends_free
    assert ef.xdrop_replay_bytes(20000, 20000, 1024) == 12830528
    assert ef.trace_bytes_long(20000, 20000) == 200000000
    assert ef.xdrop_replay_bytes(2100, 2100, 1024) == 689840
    assert ef.trace_bytes_long(2100, 2100) == 2217600
    assert ef.xdrop_replay_bytes(1100, 1070, 64) == 574208
    # derived, not measured: pairs of 20,000 x 20,000 per 1 GiB trace chunk
    assert (1 << 30) // 200000000 == 5 and (1 << 30) // 12830528 == 83


def test_class_pairs_and_empty_sequences(saln):
    ef = saln.ends_free
    for R in (0,) + TILE_ROWS:
        assert ef.xdrop_replay_bytes(0, 0, R) == ef.xdrop_replay_bytes(0, 70000, R) == 0
        assert ef.xdrop_replay_bytes(5000, 0, R) == 0
        for n in (1, 160, 161, 512, 513, 1024):
            for m in (1, 63, 300, 65000):
                assert ef.xdrop_replay_bytes(n, m, R) == ef.trace_bytes(n, m), (n, m, R)


def test_the_footprint_is_the_formula(saln):
    ef = saln.ends_free
    for R in TILE_ROWS:
        for n in (1024, 1025, 2048, 2049):
            for m in (R, R + 1, 65000, 65001):
                if n <= 1024 and m <= 65000:
                    assert ef.xdrop_replay_bytes(n, m, R) == ef.trace_bytes(n, m), (n, m, R)
                else:
                    b = ef.xdrop_replay_bytes(n, m, R)
                    assert b == footprint(n, m, R) and b % 16 == 0, (n, m, R)
    assert footprint(1025, 64, 64) == 2 * 16 + 64 * 16 + 0 + 64 * 512       # no checkpoint row at m = R
    assert footprint(1025, 65, 64) == 2 * 16 + 65 * 16 + 2 * 1024 * 16 + 64 * 512


def test_tile_rows_0_reads_the_option_and_100_is_refused(saln, saln_opt):
    from sequencealigning_amd import _lib
    ef = saln.ends_free
    R = _lib.get_option("ends_free.tile_rows")[0]
    assert ef.xdrop_replay_bytes(3000, 200) == ef.xdrop_replay_bytes(3000, 200, R) == footprint(3000, 200, R)
    saln_opt("ends_free.tile_rows", 64)
    assert ef.xdrop_replay_bytes(3000, 200) == footprint(3000, 200, 64) != footprint(3000, 200, R)
    for n, m in ((3000, 200), (100, 100)):
        with pytest.raises(_lib.SalnError) as err:
            ef.xdrop_replay_bytes(n, m, 100)
        assert err.value.code == _lib.E_INVALID and "tile_rows" in _lib.last_error()
    with pytest.raises(_lib.SalnError):
        ef.xdrop_replay_bytes((1 << 30) - 2 - 70000, 70000, 64)      # as saln_ends_free_replay_bytes


# ---------------------------------------------------------------- the refusals, host only
class Calls:
    def __init__(self):
        from sequencealigning_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.ctx_mem = C.create_string_buffer(1 << 14)      # stands for a context without overrides
        self.ctx = C.cast(self.ctx_mem, C.c_void_p)

    def batch(self, len_q, len_db, xdrop, matrix=False, scoring=None):
        qo, do = np.array([0, len_q], np.uint64), np.array([0, len_db], np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out = C.c_void_p()
        if matrix is False:
            f, sarg = self.L.saln_ends_free_xdrop_replay_align_batch, self.lib.scoring_arg(scoring)
        else:
            f, sarg = self.L.saln_ends_free_sub_xdrop_replay_align_batch, matrix
        rc = f(self.ctx, None, vp(qo), 1, None, vp(do), 1, None, None, 1, sarg, xdrop, 0, 1, C.byref(out))
        assert not out.value
        return rc, self.lib.last_error()


@pytest.fixture(scope="module")
def calls(saln):
    return Calls()


def _matrix(saln):
    return C.pointer(saln.SubstitutionMatrix(b"ACGT", ASYM, -5, -2).c_struct())


def test_a_negative_x_is_refused(saln, calls):
    from sequencealigning_amd import _lib
    for matrix in (False, _matrix(saln)):
        rc, msg = calls.batch(3000, 70000, -1, matrix)
        assert rc == _lib.E_INVALID and "negative" in msg, msg


def test_the_first_x_outside_the_guard_is_refused(saln, calls):
    """(3,000 + 70,000 + 2) * 8 = 584,016 under both scorings (the matrix's
    largest magnitude is 8): X = 2^30 - 584,016 is the first outside."""
    from sequencealigning_amd import _lib
    for matrix in (False, _matrix(saln)):
        rc, msg = calls.batch(3000, 70000, (1 << 30) - 584016, matrix)
        assert rc == _lib.E_INVALID and "xdrop reaches 2^30" in msg, msg


def test_a_null_matrix_is_refused(saln, calls):
    from sequencealigning_amd import _lib
    rc, msg = calls.batch(3000, 10, 50, matrix=None)
    assert rc == _lib.E_INVALID and "NULL" in msg, msg


def test_tile_rows_100_is_refused(saln, calls, saln_opt):
    from sequencealigning_amd import _lib
    saln_opt("ends_free.tile_rows", 100)
    for matrix in (False, _matrix(saln)):
        rc, msg = calls.batch(3000, 70000, 50, matrix)
        assert rc == _lib.E_INVALID and "tile_rows" in msg and "100" in msg, msg


def test_python_refuses_a_float_x(saln):
    ef = saln.ends_free
    with pytest.raises(ValueError, match="integer"):
        ef.xdrop_extend_long_batch([b"ACGT"], [b"ACGT"], xdrop=2.5, replay=True)
    with pytest.raises(ValueError, match="integer"):
        ef.xdrop_extend_long(b"ACGT", b"ACGT", xdrop=2.5, replay=True)
