"""Throughput of the chunked ends-free fill (saln_ends_free_long_align_batch,
ends_free_long_kernels.hip) next to the 64 x 16 class fill it decomposes.

    python tools/bench_ends_free_long.py [--pairs 4096] [--steps 10] [--warmup 2] [--alternations 3]

Workloads (G-mut(5%) pairs, `distinct` generated pairs drawn round-robin), all
timed as the wall clock of the C call, host buffers in, records out:
  local / semi-global 2,048 x 2,000, score only   the chunked fill, two chunks
      yardstick, in the same process in alternation: saln_ends_free_align_batch
      on twice as many 1,024 x 2,000 pairs, the two halves of every query
      against the same db: equal cells, the 64 x 16 class fill
  one lone local 20,000 x 20,000 pair with CIGAR  the chunked fill, 20 chunks
GCUPS = len_q * len_db * pairs / time.  A sample of the 2,048 x 2,000 pairs is
compared with tests/ends_free_model.py; the lone pair's score and end with the
linear-memory model of tests/test_ends_free_long.py, and its CIGAR with itself
(score, lengths).  Prints one JSON line and writes it, with every sample, to
--out (default profiles/ends_free_long_bench.json).
"""
import argparse
import json
import os

import numpy as np

from ends_free_bench_util import ROOT, batch_call, long_pairs, model_check, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096, help="2,048 x 2,000 pairs of a batch")
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="pairs per workload checked against the model")
    ap.add_argument("--lone", type=int, default=20000, help="side of the lone pair (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_free_long_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import synth
    from test_ends_free_long import linear_ends

    ef = saln.ends_free
    lq, ld = 2048, 2000
    seed = 0x5EED10F6
    qs, ds = long_pairs(synth, a.distinct, seed, lq, ld)
    halves = [h for q in qs for h in (q[:1024], q[1024:])]
    assert ef.pair_path_long(lq, ld) == (1, 2) and ef.pair_path_long(1024, ld) == (0, 1)
    q_seq, q_off = saln.pack_csr(qs)
    h_seq, h_off = saln.pack_csr(halves)
    d_seq, d_off = saln.pack_csr(ds)
    idx = np.arange(a.pairs, dtype=np.uint32) % np.uint32(a.distinct)
    hq = np.ascontiguousarray(np.stack([2 * idx, 2 * idx + 1], 1).reshape(-1))
    hd = np.ascontiguousarray(np.repeat(idx, 2))
    cells = float(lq) * ld * a.pairs

    out = {"pairs": a.pairs, "distinct": a.distinct, "steps": a.steps, "warmup": a.warmup,
           "alternations": a.alternations, "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, mode in (("local 2048x2000 score only", 1), ("semi-global 2048x2000 score only", 2)):
        run_long = batch_call("saln_ends_free_long_align_batch", q_seq, q_off, d_seq, d_off, idx, idx, mode, None, 0)
        run_cls = batch_call("saln_ends_free_align_batch", h_seq, h_off, d_seq, d_off, hq, hd, mode, None, 0)
        t_long, t_cls = [], []
        for _ in range(a.alternations):
            t_long += wall_ms(run_long, a.warmup, a.steps)
            t_cls += wall_ms(run_cls, a.warmup, a.steps)
        k = min(a.check, a.distinct)
        got, _ = ef.ends_free_align_long_batch(qs[:k], ds[:k], [(j, j) for j in range(k)], mode=mode,
                                               cigar=False)
        ok = model_check(got, None, qs, ds, mode, None, False)
        med_long, med_cls = float(np.median(t_long)), float(np.median(t_cls))
        out["workloads"].append({
            "name": name, "timing": "host buffers in, records out, wall clock of the C call",
            "len_q": lq, "len_db": ld, "pairs": a.pairs,
            "long_ms": round(med_long, 3), "long_gcups": round(cells / med_long / 1e6, 1),
            "class_fill_pairs": 2 * a.pairs, "class_fill_len_q": 1024,
            "class_fill_ms": round(med_cls, 3), "class_fill_gcups": round(cells / med_cls / 1e6, 1),
            "ratio_long_over_class_fill": round(med_cls / med_long, 3),
            "long_ms_samples": [round(t, 3) for t in t_long],
            "class_fill_ms_samples": [round(t, 3) for t in t_cls],
            "model_check": {"pairs": k, "ok": ok},
        })
    if a.lone:
        n = a.lone
        q = synth.random_bases(seed ^ 0x10E, n).tobytes()
        d = synth.mutate(q, 0.05, seed=77)
        d = (d + synth.random_bases(seed ^ 0x20E, n).tobytes())[:n]
        lone = {}

        def run_lone():
            lone["res"], lone["cig"] = ef.local_align_long(q, d)

        ts = []
        for _ in range(a.alternations):
            ts += wall_ms(run_lone, a.warmup, a.steps)
        r, cigar = lone["res"], lone["cig"]
        score, q_end, db_end = linear_ends(q, d, 1)
        ok = (int(r["score"]), int(r["q_end"]), int(r["db_end"])) == (score, q_end, db_end)
        ok &= ef.cigar_score(cigar) == score
        ok &= sum(k for k, op in cigar if op in "=XI") == q_end - int(r["q_begin"])
        ok &= sum(k for k, op in cigar if op in "=XD") == db_end - int(r["db_begin"])
        med = float(np.median(ts))
        out["workloads"].append({
            "name": f"local {n}x{n} lone pair with CIGAR",
            "timing": "host buffers in, CIGAR out, wall clock of local_align_long",
            "len_q": n, "len_db": len(d), "pairs": 1, "chunks": ef.pair_path_long(n, len(d))[1],
            "long_ms": round(med, 3), "long_gcups": round(float(n) * len(d) / med / 1e6, 2),
            "long_ms_samples": [round(t, 3) for t in ts],
            "record": [int(v) for v in r], "model_check": {"pairs": 1, "ok": bool(ok)},
        })
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(w["model_check"]["ok"] for w in out["workloads"]):
        raise SystemExit("model check failed")


if __name__ == "__main__":
    main()
