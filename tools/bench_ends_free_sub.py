"""Throughput of the ends-free fills under a substitution matrix
(saln_ends_free_sub_*, the kSub kernel instances) next to the scalar scoring on
the same pairs.

    python tools/bench_ends_free_sub.py [--cells 2.5e9] [--steps 10] [--warmup 2] [--alternations 3]

Per fill, local mode, score only (G-mut(5%) pairs, `distinct` generated pairs
drawn round-robin):
  scalar   scoring (5, -4, -8, -6), the instances without kSub
  matrix   a 4-symbol matrix over ACGT that encodes the same scoring, on the
           same pairs: the records must be equal, the time ratio is the cost
           of the table lookup
  protein  a 24-symbol protein-shaped matrix (a symbol against itself 4 .. 11,
           against another -8 .. 2, asymmetric) on 24-letter pairs of the same
           shape, 10 % substituted
The class fills (150 x 150: 16 x 10; 250 x 250: 16 x 16; 500 x 500: 64 x 8;
1,000 x 1,000: 64 x 16) run as EndsFreePlan, device resident, timed with
hipEvents; the chunked fill (2,048 x 2,000) as the wall clock of the C call,
host buffers in, records out.  The three are measured in alternation in the
same process.  GCUPS = len_q * len_db * pairs / time.  A sample of the protein
pairs is compared with tests/ends_free_model.py.  Prints one JSON line and
writes it, with every sample, to --out (default
profiles/ends_free_sub_bench.json).
"""
import argparse
import json
import os
import random

import numpy as np

from ends_free_bench_util import ROOT, events_ms, wall_ms

SCALAR = (5, -4, -8, -6)
PROTEIN = b"ARNDCQEGHILKMFPSTWYVBZXU"


def _protein_pairs(distinct, lq, ld, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(PROTEIN, np.uint8)
    qs, ds = [], []
    for _ in range(distinct):
        q = letters[rng.integers(0, 24, lq)]
        d = np.resize(q, ld).copy()
        hit = rng.random(ld) < 0.10
        d[hit] = letters[rng.integers(0, 24, int(hit.sum()))]
        qs.append(q.tobytes())
        ds.append(d.tobytes())
    return qs, ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=float, default=2.5e9, help="cells of a class-fill batch")
    ap.add_argument("--long-pairs", type=int, default=2048, help="2,048 x 2,000 pairs of a batch")
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="protein pairs per workload checked against the model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_free_sub_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import synth
    import ends_free_model as model

    ef = saln.ends_free
    table4 = [[SCALAR[0] if x == y else SCALAR[1] for y in range(4)] for x in range(4)]
    sm4 = saln.SubstitutionMatrix(b"ACGT", table4, SCALAR[2], SCALAR[3])
    rng = random.Random(0x24B2)
    table24 = [[rng.randint(4, 11) if x == y else rng.randint(-8, 2) for y in range(24)] for x in range(24)]
    sm24 = saln.SubstitutionMatrix(PROTEIN, table24, -10, -2)
    msc24 = model.matrix_scoring(PROTEIN, table24, -10, -2)
    mode = 1
    out = {"cells": a.cells, "long_pairs": a.long_pairs, "distinct": a.distinct, "steps": a.steps,
           "warmup": a.warmup, "alternations": a.alternations, "mode": "local, score only",
           "device": torch.cuda.get_device_name(0), "workloads": []}
    shapes = [(150, 150, False), (250, 250, False), (500, 500, False), (1000, 1000, False), (2048, 2000, True)]
    for lq, ld, chunked in shapes:
        n_pairs = a.long_pairs if chunked else max(a.distinct, int(a.cells / (lq * ld)))
        seed = 0x5EED5B00 + lq
        allq = synth.random_bases(seed, a.distinct * lq).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(a.distinct)]
        ds = [(synth.mutate(q, 0.05, seed=k) + q)[:ld] for k, q in enumerate(qs)]
        pq, pd = _protein_pairs(a.distinct, lq, ld, seed)
        idx = np.arange(n_pairs, dtype=np.uint32) % np.uint32(a.distinct)
        pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
        cells = float(lq) * ld * n_pairs
        assert ef.pair_path_long(lq, ld)[0] == int(chunked)
        runs, last = {}, {}
        if chunked:
            for name, seqs, sc in (("scalar", (qs, ds), SCALAR), ("matrix", (qs, ds), sm4),
                                   ("protein", (pq, pd), sm24)):
                def run(name=name, seqs=seqs, sc=sc):
                    last[name] = ef.ends_free_align_long_batch(seqs[0], seqs[1], pairs, mode=mode, scoring=sc,
                                                               cigar=False)[0]
                runs[name] = run
            timer, how = wall_ms, "host buffers in, records out, wall clock of ends_free_align_long_batch"
        else:
            keep = []
            for name, seqs, sc in (("scalar", (qs, ds), SCALAR), ("matrix", (qs, ds), sm4),
                                   ("protein", (pq, pd), sm24)):
                q_seq, q_off = saln.pack_csr(seqs[0])
                d_seq, d_off = saln.pack_csr(seqs[1])
                dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
                dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
                plan = ef.EndsFreePlan(q_off, d_off, pairs, mode=mode, scoring=sc)
                res = torch.zeros(n_pairs * 8, dtype=torch.int32, device="cuda")
                keep.append(plan)
                last[name] = res
                runs[name] = lambda plan=plan, dq=dq, dd=dd, res=res: plan.execute(dq, dd, res)
            timer, how = events_ms, "EndsFreePlan, device resident, hipEvents"
        ts = {name: [] for name in runs}
        for _ in range(a.alternations):
            for name, run in runs.items():
                ts[name] += timer(run, a.warmup, a.steps)
        if chunked:
            got = {name: np.asarray(v) for name, v in last.items()}
        else:
            from sequencealigning_amd import _lib
            torch.cuda.synchronize()
            got = {name: v.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE) for name, v in last.items()}
            for plan in keep:
                plan.close()
        equal = bool((got["scalar"] == got["matrix"]).all())
        k = min(a.check, a.distinct)
        ok = all((int(got["protein"]["score"][j]), int(got["protein"]["q_end"][j]),
                  int(got["protein"]["db_end"][j])) == model.linear_ends(pq[j], pd[j], mode, msc24)
                 for j in range(k))
        med = {name: float(np.median(v)) for name, v in ts.items()}
        w = {"len_q": lq, "len_db": ld, "pairs": n_pairs, "timing": how,
             "fill": "chunked" if chunked else "%d x %d" % ef.pair_geometry(lq),
             "matrix_equals_scalar": equal, "model_check": {"pairs": k, "ok": bool(ok)},
             "ratio_matrix_over_scalar_time": round(med["matrix"] / med["scalar"], 3),
             "ratio_protein_over_scalar_time": round(med["protein"] / med["scalar"], 3)}
        for name in runs:
            w[name + "_ms"] = round(med[name], 3)
            w[name + "_gcups"] = round(cells / med[name] / 1e6, 1)
            w[name + "_ms_samples"] = [round(t, 3) for t in ts[name]]
        out["workloads"].append(w)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(w["model_check"]["ok"] and w["matrix_equals_scalar"] for w in out["workloads"]):
        raise SystemExit("check failed")


if __name__ == "__main__":
    main()
