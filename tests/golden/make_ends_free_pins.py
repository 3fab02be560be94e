"""Writes ends_free_model_pins.json: what tests/ends_free_model.py answers on
40 stored pairs per scoring, in the four modes.  Brute force pins the model's
scores; this file pins its canonical choices (the smallest i, then j; a
last-column cell over a last-row cell; the first of M, I, D; extend before
open), which test_ends_free_model.py::test_pins holds it to.

The file was first written from the four separate models this one replaced
(local and semi-global, overlap, substitution matrix, extend), through an
adapter with this module's interface; the one model regenerates it byte for
byte.  Regenerate with:
    python tests/golden/make_ends_free_pins.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ends_free_model as model  # noqa: E402

MODES = [model.LOCAL, model.SEMI_GLOBAL, model.OVERLAP, model.EXTEND]
SCHEMES = [(5, -4, -8, -6), (1, -1, 0, -1), (2, -3, -5, -2)]
# test_ends_free_sub_model.py's three symbols, so 'T' is the byte outside the alphabet
ALPHABET3, TABLE3 = "ACG", [[4, -3, 2], [-2, 3, 0], [-4, -5, -1]]
GAPS3 = [(-3, -1), (0, -2)]


def make_pairs(seed):
    """q of 0..24 bytes, d of 0..36; every other pair over AC (ties are
    common), the rest over ACGT; every third has the query's last 8 bytes at
    the db's start, every fifth (that is no third) its first 12; pairs 1, 2 and 4
    are the empty query, the empty db and both."""
    rng = random.Random(seed)
    pairs = []
    for k in range(40):
        alphabet = "AC" if k % 2 else "ACGT"
        q = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 24)))
        d = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 36)))
        if k == 1:
            q, d = "", d or "A"
        elif k == 2:
            q, d = q or "A", ""
        elif k == 4:
            q = d = ""
        elif k % 3 == 0:
            d = (q[-8:] + d)[:36]
        elif k % 5 == 0:
            d = (q[:12] + d)[:36]
        pairs.append([q, d])
    return pairs


def scoring_of(spec):
    """A fixture entry's "scoring": a 4-list, or a matrix with its gap pair."""
    if isinstance(spec, list):
        return tuple(spec)
    return model.matrix_scoring(spec["alphabet"].encode(), spec["table"], spec["o"], spec["e"])


def cigar_string(cigar):
    return "".join(f"{n}{op}" for n, op in cigar)


def main():
    specs = [list(s) for s in SCHEMES] + [
        {"alphabet": ALPHABET3, "table": TABLE3, "o": o, "e": e} for o, e in GAPS3]
    out = []
    for k, spec in enumerate(specs):
        sc, pairs = scoring_of(spec), make_pairs(0xE1F + k)
        expected = {}
        for mode in MODES:
            rows = []
            for q, d in pairs:
                a = model.align(q.encode(), d.encode(), mode, sc)
                rows.append([list(a.record()), cigar_string(a.cigar)])
            expected[str(mode)] = rows
        out.append({"scoring": spec, "pairs": pairs, "expected": expected})
    with open(os.path.join(HERE, "ends_free_model_pins.json"), "w") as f:
        json.dump({"source": "tests/ends_free_model.py via tests/golden/make_ends_free_pins.py",
                   "record": "score, status, q_begin, q_end, db_begin, db_end, cigar_len, reserved",
                   "scorings": out}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
