"""CPU, no device: the plain model of overlap (dovetail) alignment
(ends_free_model.py, OVERLAP) against brute-force enumeration, its tie rules on hand
cases, its place between semi-global and local, and the host-only ABI the new
mode must leave alone."""
import itertools
import os
import random
import re
from functools import lru_cache

import ends_free_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the engine's three test schemes and one whose mismatch is worse than o + e
SCHEMES = [(5, -4, -8, -6), (1, -1, 0, -1), (2, -3, -5, -2), (4, -9, 0, -1)]


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ------------------------------------------------------------------ brute force
def brute_counts(q: bytes, d: bytes):
    """Every alignment that starts on row 0 or column 0 and ends on row m or
    column n, an I run and a D run never adjacent, as the set of its (matches,
    mismatches, gap runs, gap columns): enumeration by steps, no maximum
    anywhere, so a scheme's best score is a plain max over the set."""
    n, m = len(q), len(d)

    @lru_cache(maxsize=None)
    def tails(i, j, last):
        """Counts of every way on from (i, j), the step into it being `last`."""
        out = set()
        if i == m or j == n:
            out.add((0, 0, 0, 0))          # the alignment may end here
        if i < m and j < n:
            same = q[j] == d[i]
            for a, b, g, l in tails(i + 1, j + 1, "M"):
                out.add((a + same, b + (not same), g, l))
        if j < n and last != "D":
            for a, b, g, l in tails(i, j + 1, "I"):
                out.add((a, b, g + (last != "I"), l + 1))
        if i < m and last != "I":
            for a, b, g, l in tails(i + 1, j, "D"):
                out.add((a, b, g + (last != "D"), l + 1))
        return frozenset(out)

    starts = [(i, 0) for i in range(m + 1)] + [(0, j) for j in range(1, n + 1)]
    return set().union(*(tails(i, j, "M") for i, j in starts))


def brute_score(counts, scheme):
    ma, mi, o, e = scheme
    return max(a * ma + b * mi + g * o + l * e for a, b, g, l in counts)


def check_alignment(q, d, a, scheme):
    """The model's alignment re-scores to its score and spans its ranges."""
    ma, mi, o, e = scheme
    n, m = len(q), len(d)
    if a.score == 0:
        assert a.record() == (0, 0, 0, 0, 0, 0, 0, 0)
        return
    assert a.score > 0 and a.cigar
    assert a.q_begin == 0 or a.db_begin == 0
    assert a.q_end == n or a.db_end == m
    i, j, total, prev = a.db_begin, a.q_begin, 0, None
    for k, op in a.cigar:
        assert k > 0 and op != prev
        assert not (prev in ("I", "D") and op in ("I", "D")), a.cigar
        if op in "=X":
            for t in range(k):
                assert (q[j + t] == d[i + t]) == (op == "="), (a.cigar, i, j)
            total += k * (ma if op == "=" else mi)
            i, j = i + k, j + k
        elif op == "I":
            total += o + k * e
            j += k
        else:
            total += o + k * e
            i += k
        prev = op
    assert (i, j) == (a.db_end, a.q_end)
    assert total == a.score


def _check_pair(q, d):
    counts = brute_counts(q, d)
    for scheme in SCHEMES:
        a = model.align(q, d, model.OVERLAP, scheme)
        assert a.score == brute_score(counts, scheme), (q, d, scheme)
        check_alignment(q, d, a, scheme)
        b = model.align(q, d, model.OVERLAP, scheme, walk=False)
        want = (a.score, -1, a.q_end, -1, a.db_end) if a.score else (0, -1, 0, -1, 0)
        assert (b.score, b.q_begin, b.q_end, b.db_begin, b.db_end) == want and b.cigar == []
        assert model.linear_ends(q, d, model.OVERLAP, scheme) == (a.score, a.q_end, a.db_end), (q, d, scheme)
        # between the engine's other modes: both semi-global end sets lie on
        # overlap's two borders, and a local alignment may drop any overhang
        local = model.align(q, d, model.LOCAL, scheme, walk=False).score
        semi_qd = model.align(q, d, model.SEMI_GLOBAL, scheme, walk=False).score
        semi_dq = model.align(d, q, model.SEMI_GLOBAL, scheme, walk=False).score
        assert max(semi_qd, semi_dq) <= a.score <= local, (q, d, scheme)


def test_all_pairs_over_ac_up_to_4x4():
    seqs = [bytes(t) for k in range(5) for t in itertools.product(b"AC", repeat=k)]
    assert len(seqs) == 31
    for q in seqs:
        for d in seqs:
            _check_pair(q, d)


def test_random_pairs_up_to_6x6():
    rng = random.Random(0x0E71)
    for _ in range(150):
        alphabet = rng.choice([b"AC", b"ACGT"])
        _check_pair(_rand(rng, rng.randint(0, 6), alphabet), _rand(rng, rng.randint(0, 6), alphabet))


def test_harsh_mismatch_scheme_is_harsh():
    ma, mi, o, e = SCHEMES[3]
    assert mi < o + e      # a gap of one column is cheaper than a mismatch


# ------------------------------------------------------------------ hand cases
def test_dovetails_and_containments():
    a = model.align(b"TTTTACGTA", b"ACGTACCCC", model.OVERLAP)          # query suffix over db prefix
    assert a.record() == (25, 0, 4, 9, 0, 5, 1, 0) and a.cigar == [(5, "=")]
    a = model.align(b"ACGTACCCC", b"TTTTACGTA", model.OVERLAP)          # db suffix over query prefix
    assert a.record() == (25, 0, 0, 5, 4, 9, 1, 0)
    a = model.align(b"ACGTAC", b"GGGACGTACGGG", model.OVERLAP)          # the query inside the db
    assert a.record() == (30, 0, 0, 6, 3, 9, 1, 0)
    a = model.align(b"GGGACGTACGGG", b"ACGTAC", model.OVERLAP)          # the db inside the query
    assert a.record() == (30, 0, 3, 9, 0, 6, 1, 0)
    a = model.align(b"ACGTACGT", b"ACGTACGT", model.OVERLAP)
    assert a.record() == (40, 0, 0, 8, 0, 8, 1, 0)
    for q, d in ((b"AAAA", b"CCCCCC"), (b"", b"ACGT"), (b"ACGT", b""), (b"", b""), (b"A", b"C")):
        assert model.align(q, d, model.OVERLAP).record() == (0, 0, 0, 0, 0, 0, 0, 0)
        assert model.align(q, d, model.OVERLAP, walk=False).record() == (0, 0, -1, 0, -1, 0, 0, 0)
    assert model.align(b"A", b"A", model.OVERLAP).record() == (5, 0, 0, 1, 0, 1, 1, 0)


def test_tie_rules():
    # a last-column cell above row m against a last-row cell: the smaller row
    info = model.end_info(b"ACTTTTAC", b"ACGGGGAC")
    assert info["col_ties"] == [2] and info["row_ties"] == [2]
    assert model.align(b"ACTTTTAC", b"ACGGGGAC", model.OVERLAP).record() == (10, 0, 6, 8, 0, 2, 1, 0)
    # two last-row cells, one of them the corner: the smaller column
    info = model.end_info(b"ACTAC", b"AC")
    assert info["row_ties"] == [2, 5] and info["col_ties"] == [2]
    assert model.align(b"ACTAC", b"AC", model.OVERLAP).record() == (10, 0, 0, 2, 0, 2, 1, 0)
    # two last-column cells, one of them the corner: the smaller row
    info = model.end_info(b"AC", b"ACTAC")
    assert info["col_ties"] == [2, 5] and info["row_ties"] == [2]
    assert model.align(b"AC", b"ACTAC", model.OVERLAP).record() == (10, 0, 0, 2, 0, 2, 1, 0)


def test_end_states_and_gap_exits():
    """Under the harsh scheme a one-column gap beats a mismatch, so an
    alignment may end in I or D and may leave through a gap that opened from
    the free start (an 'I' into column 0, a 'D' into row 0)."""
    sc = SCHEMES[3]
    cases = [   # q, d, end state, record, cigar
        (b"ACA", b"CC", "I", (3, 0, 1, 3, 0, 1, 2, 0), [(1, "="), (1, "I")]),
        (b"AAA", b"CCAC", "D", (3, 0, 0, 1, 2, 4, 2, 0), [(1, "="), (1, "D")]),
        (b"AA", b"CAC", "M", (3, 0, 0, 2, 1, 2, 2, 0), [(1, "I"), (1, "=")]),
        (b"AAA", b"CAC", "M", (3, 0, 2, 3, 0, 2, 2, 0), [(1, "D"), (1, "=")]),
    ]
    for q, d, st, rec, cigar in cases:
        a = model.align(q, d, model.OVERLAP, sc)
        assert (model.end_info(q, d, sc)["st"], a.record(), a.cigar) == (st, rec, cigar), (q, d)
        check_alignment(q, d, a, sc)
        assert a.score == brute_score(brute_counts(q, d), sc)


# ------------------------------------------------------------------ host-only ABI
def test_mode_constant_matches_the_header(saln):
    src = open(os.path.join(ROOT, "include", "saln.h")).read()
    assert int(re.search(r"SALN_MODE_OVERLAP = (\d+)", src).group(1)) == saln.ends_free.OVERLAP == 4
    assert model.OVERLAP == 4
    assert [int(v) for v in re.findall(r"SALN_MODE_[A-Z_]+ = (\d+)", src)] == [0, 1, 2, 4]
    assert not hasattr(saln.Mode, "Overlap") and len(saln.Mode) == 3
    assert saln.overlap_align is saln.ends_free.overlap_align
    assert saln.overlap_align_long is saln.ends_free.overlap_align_long


def test_host_only_sizes_do_not_know_the_mode(saln):
    """trace_bytes, pair_geometry and pair_path_long take no mode: the values
    DESIGN.md section 3c/3d give."""
    ef = saln.ends_free
    assert [ef.pair_geometry(n) for n in (1, 160, 161, 256, 257, 512, 513, 1024)] == [
        (16, 10), (16, 10), (16, 16), (16, 16), (64, 8), (64, 8), (64, 16), (64, 16)]
    assert ef.trace_bytes(150, 400) == 400 * 75
    assert ef.trace_bytes(1024, 3) == 3 * 512 and ef.trace_bytes(161, 1) == 88
    assert ef.trace_bytes_long(2048, 2000) == 2000 * 1024
    assert ef.pair_path_long(1024, 65000) == (0, 1) and ef.pair_path_long(2500, 7) == (1, 3)
    assert ef.pair_path_long(100, 65001) == (1, 1)
