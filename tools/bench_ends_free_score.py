"""Throughput of the score-only search (EndsFreeScorePlan: the packed-i16 fill,
two pairs per lane group) next to the engine's i32 score-only plan
(EndsFreePlan) on the same pairs and scoring.

    python tools/bench_ends_free_score.py [--pairs 100000] [--steps 10] [--warmup 2] [--alternations 3]

Workloads (`distinct` generated pairs drawn round-robin):
  local 150x150 scalar            G-mut(5%) pairs
  semi-global 150x400 scalar      the read's mutated copy inside a random window
  local 300x350 matrix            20 letters under a matrix built here (no matrix file ships)
  local 1000x1000 scalar          a tenth of the pairs
Both sides are device-resident plans timed by hipEvents, in one process and in
alternation.  GCUPS = len_q * len_db * pairs / time.  A sample of every
workload is checked against tests/ends_free_model.py, and every score of the
two plans against each other.  `faster_beyond_spread`: the packed plan's
slowest sample lies below the i32 plan's fastest.  Prints one JSON line.
"""
import argparse
import json

import numpy as np

from ends_free_bench_util import events_ms, short_pairs

LETTERS = b"ARNDCQEGHILKMFPSTWYV"


def bench_matrix(saln):
    """A BLOSUM-shaped table: symmetric, 4 .. 11 on the diagonal, -4 .. 3 off it."""
    rng = np.random.default_rng(0x5EEDB10)
    n = len(LETTERS)
    t = rng.integers(-4, 4, size=(n, n))
    t = np.triu(t, 1) + np.triu(t, 1).T + np.diag(rng.integers(4, 12, size=n))
    return saln.SubstitutionMatrix(LETTERS, t.tolist(), -11, -1), t.tolist()


def protein_pairs(distinct, lq, ld, seed=0x5EED0507):
    """Queries over 20 letters; a db is its query with 10 % of the letters
    replaced, inside random letters."""
    rng = np.random.default_rng(seed)
    sym = np.frombuffer(LETTERS, np.uint8)
    qs, ds = [], []
    for _ in range(distinct):
        q = sym[rng.integers(0, len(sym), lq)]
        d = sym[rng.integers(0, len(sym), ld)].copy()
        m = q.copy()
        hit = rng.random(lq) < 0.10
        m[hit] = sym[rng.integers(0, len(sym), int(hit.sum()))]
        at = int(rng.integers(0, ld - lq + 1))
        d[at:at + lq] = m
        qs.append(q.tobytes())
        ds.append(d.tobytes())
    return qs, ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=24, help="pairs per workload checked against the model")
    a = ap.parse_args()
    assert a.steps >= 10 and a.alternations >= 3, "at least 10 timed steps and 3 alternations"
    import torch
    import ends_free_model as model
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    matrix, table = bench_matrix(saln)
    mscoring = model.matrix_scoring(LETTERS, table, -11, -1)
    out = {"pairs": a.pairs, "steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "timing": "device resident plans, hipEvents, the two sides in alternation",
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, mode, lq, ld, scoring, msc, pairs_n in (
            ("local 150x150 scalar", 1, 150, 150, None, None, a.pairs),
            ("semi-global 150x400 scalar", 2, 150, 400, None, None, a.pairs),
            ("local 300x350 matrix", 1, 300, 350, matrix, mscoring, a.pairs),
            ("local 1000x1000 scalar", 1, 1000, 1000, None, None, max(1, a.pairs // 10))):
        seed = 0x5EED0E0F
        if scoring is not None:
            qs, ds = protein_pairs(a.distinct, lq, ld)
        elif ld == lq:
            allq = synth.random_bases(seed, a.distinct * lq).tobytes()
            qs = [allq[k * lq:(k + 1) * lq] for k in range(a.distinct)]
            ds = [(synth.mutate(q, 0.05, seed=k) + q)[:ld] for k, q in enumerate(qs)]
        else:
            qs, ds = short_pairs(synth, a.distinct, seed, lq, ld)
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.arange(pairs_n, dtype=np.uint32) % np.uint32(a.distinct)
        pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
        cells = float(lq) * ld * pairs_n
        dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
        dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
        pk_plan = ef.EndsFreeScorePlan(q_off, d_off, pairs, mode=mode, scoring=scoring)
        i32_plan = ef.EndsFreePlan(q_off, d_off, pairs, mode=mode, scoring=scoring)
        scores = torch.zeros(pairs_n, dtype=torch.int32, device="cuda")
        res = torch.zeros(pairs_n * 8, dtype=torch.int32, device="cuda")
        run_pk = lambda: pk_plan.execute(dq, dd, scores)               # noqa: E731
        run_i32 = lambda: i32_plan.execute(dq, dd, res)                # noqa: E731
        t_pk, t_i32 = [], []
        for _ in range(a.alternations):
            t_pk += events_ms(run_pk, a.warmup, a.steps)
            t_i32 += events_ms(run_i32, a.warmup, a.steps)
        torch.cuda.synchronize()
        got = scores.cpu().numpy()
        ref = res.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE)["score"]
        k = min(a.check, a.distinct, pairs_n)
        ok = all(int(got[j]) == model.linear_ends(qs[j], ds[j], mode, msc)[0] for j in range(k))
        med_pk, med_i32 = float(np.median(t_pk)), float(np.median(t_i32))
        out["workloads"].append({
            "name": name, "len_q": lq, "len_db": ld, "pairs": pairs_n,
            "packed_pairs_i32_pairs": list(pk_plan.info()),
            "score_ms": round(med_pk, 3), "score_gcups": round(cells / med_pk / 1e6, 1),
            "score_ms_min_max": [round(min(t_pk), 3), round(max(t_pk), 3)],
            "i32_ms": round(med_i32, 3), "i32_gcups": round(cells / med_i32 / 1e6, 1),
            "i32_ms_min_max": [round(min(t_i32), 3), round(max(t_i32), 3)],
            "ratio_score_over_i32": round(med_i32 / med_pk, 3),
            "faster_beyond_spread": bool(max(t_pk) < min(t_i32)),
            "samples_each": len(t_pk), "scores_equal_i32": bool((got == ref).all()),
            "model_check": {"pairs": k, "ok": bool(ok)},
        })
        pk_plan.close()
        i32_plan.close()
    print(json.dumps(out))
    if not all(w["model_check"]["ok"] and w["scores_equal_i32"] for w in out["workloads"]):
        raise SystemExit("check failed")


if __name__ == "__main__":
    main()
