"""CPU: facts about the reference WFA (oracle/refwfa.c) that the engine's two
caps (max_steps, max_width; include/saln.h) and its GPU tests
(test_wfa_caps_gpu.py) rely on."""
import itertools

import pytest

from wfa_check import seeded_pairs, width_cap_step, widths

A21 = (b"A" * 21, b"C")


@pytest.mark.parametrize("q, d, max_steps, W, want", [
    (*A21, 400, 64, 354),
    (*A21, 400, 67, 372),
    (*A21, 400, 68, None),
    (*A21, 80, 7, 24),
    (*A21, 80, 9, 36),
    (b"ACGT", b"ACGT", 80, 7, 24),
    (b"ACGT", b"ACGT", 80, 9, 30),
    (b"ACGT", b"ACGT", 80, 17, 54),
])
def test_width_cap_step_fixtures(oracle, q, d, max_steps, W, want):
    assert width_cap_step(oracle, q, d, W, max_steps) == want
    if want is not None:  # the same step whatever the cap at or above it, none below it
        assert width_cap_step(oracle, q, d, W, want) == want
        assert width_cap_step(oracle, q, d, W, want - 1) is None


def test_width_bound(oracle):
    """A tensor built by the k-th expand call is at most 2 * (k // 4) + 1
    diagonals wide: its sources lie 4, 6 and 8 steps back and each side grows
    by one.  So the default max_width of 64 cannot bind for max_steps <= 127."""
    pairs = seeded_pairs(21, 1002)
    assert len(pairs) >= 1000
    wide = 0
    for q, d in pairs:
        o = oracle.wfa(q, d, max_steps=300)
        w = widths(o.stdout)
        assert max(w, default=0) <= 2 * (o.steps // 4) + 1, (q, d)
        wide += max(w, default=0) > 9
    assert wide > 100  # the sample is not only pairs that end at once
    assert 2 * (127 // 4) + 1 <= 64


def test_traceback_never_moves(oracle):
    """The score at convergence is wfs.len(), which is odd, so every
    score - {4, 6, 8} the traceback looks up is odd and names no tensor: no
    run prints `mismatch`, `extend` or an `open` that moves, and every
    converged run ends in `ret` or `huh` with empty alignment rows.  This is
    why the kernel's movement branches (kinds 1 to 4), extend_rev /
    SALN_REF_PANIC_SLICE and the reserved[0] overflow flag have no GPU test:
    no input reaches them."""
    words = [bytes(w) for n in range(6) for w in itertools.product(b"AC", repeat=n)]
    pairs = [(q, d) for q in words for d in words]
    assert len(pairs) == 3969
    pairs += seeded_pairs(22, 1002, max_len=40)
    converged = 0
    for q, d in pairs:
        o = oracle.wfa(q, d, max_steps=100)
        assert o.status != oracle.WFA_PANIC_SLICE, (q, d)
        assert "mismatch\n" not in o.stdout and "extend\n" not in o.stdout, (q, d)
        assert o.stdout.count("open\n") == o.stdout.count("open\nhuh\n"), (q, d)
        assert o.aln_len1 == o.aln_len2 == 0, (q, d)
        if o.status == oracle.WFA_OK:
            converged += 1
            assert o.score % 2 == 1, (q, d)
            assert "\nret\n" in o.stdout or "\nhuh\n" in o.stdout, (q, d)
    assert converged > 1000
