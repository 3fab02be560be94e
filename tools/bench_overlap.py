"""Throughput of the ends-free engine's overlap mode (SALN_MODE_OVERLAP) next
to the engine's own semi-global fill on the same pairs.

    python tools/bench_overlap.py [--pairs 100000] [--long-pairs 4096] [--steps 10] [--warmup 2]
                                  [--alternations 3]

Workloads, at the shapes and with the pairs of tools/bench_ends_free.py and
tools/bench_ends_free_long.py (G-mut(5%) pairs drawn round-robin from
`distinct` generated ones):
  150 x 400 score only       EndsFreePlan, device resident, hipEvents
  150 x 400 with CIGAR       saln_ends_free_align_batch, host buffers in, CIGARs out (wall)
  2,048 x 2,000 score only   saln_ends_free_long_align_batch (the chunked fill), records out (wall)
  2,048 x 2,000 with CIGAR   the same with CIGARs, on long-pairs / 8 pairs (1 GiB of codes at 512)
Yardstick: semi-global through the same call on the same pairs, in the same
process, in alternation.  GCUPS = len_q * len_db * pairs / time.  A sample of
every workload is checked against tests/ends_free_model.py.  Prints one JSON
line and writes it, with every sample, to --out (default
profiles/overlap_bench.json).
"""
import argparse
import json
import os

import numpy as np

from ends_free_bench_util import ROOT, batch_call, events_ms, long_pairs, model_check, short_pairs, wall_ms

SEMI_GLOBAL, OVERLAP = 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000, help="150 x 400 pairs of a batch")
    ap.add_argument("--distinct", type=int, default=2_000)
    ap.add_argument("--long-pairs", type=int, default=4096, help="2,048 x 2,000 pairs of a batch")
    ap.add_argument("--long-distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="pairs per workload checked against the model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_bench.json"))
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import synth

    ef = saln.ends_free
    out = {"steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "device": torch.cuda.get_device_name(0), "yardstick": "semi-global, same call, same pairs",
           "workloads": []}
    shapes = (("150x400", short_pairs(synth, a.distinct), a.pairs, "saln_ends_free_align_batch"),
              ("2048x2000", long_pairs(synth, a.long_distinct), a.long_pairs,
               "saln_ends_free_long_align_batch"))
    for shape, (qs, ds), n_pairs, entry in shapes:
        lq, ld = len(qs[0]), len(ds[0])
        long = lq > ef.MAX_QUERY
        assert ef.pair_path_long(lq, ld)[0] == int(long)
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        for cigar in (False, True):
            n = max(1, n_pairs // 8) if long and cigar else n_pairs
            idx = np.ascontiguousarray(np.arange(n, dtype=np.uint32) % np.uint32(len(qs)))
            cells = float(lq) * ld * n
            plans = []
            if not cigar and not long:
                dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
                dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
                res = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
                pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
                plans = [ef.EndsFreePlan(q_off, d_off, pairs, mode=m) for m in (OVERLAP, SEMI_GLOBAL)]
                run = {m: (lambda p=p: p.execute(dq, dd, res)) for m, p in zip((OVERLAP, SEMI_GLOBAL), plans)}
                timer, how = events_ms, "device resident, hipEvents"
            else:
                run = {m: batch_call(entry, q_seq, q_off, d_seq, d_off, idx, idx, m, None, cigar)
                       for m in (OVERLAP, SEMI_GLOBAL)}
                timer = wall_ms
                how = "host buffers in, %s out, wall clock of the C call" % ("CIGARs" if cigar else "records")
            t_ov, t_sg = [], []
            for _ in range(a.alternations):
                t_ov += timer(run[OVERLAP], a.warmup, a.steps)
                t_sg += timer(run[SEMI_GLOBAL], a.warmup, a.steps)
            for p in plans:
                p.close()
            k = min(a.check, len(qs))
            align = ef.ends_free_align_long_batch if long else ef.ends_free_align_batch
            got, cig = align(qs[:k], ds[:k], [(j, j) for j in range(k)], mode=OVERLAP, cigar=cigar)
            ok = model_check(got, cig, qs, ds, OVERLAP, None, cigar)
            med_ov, med_sg = float(np.median(t_ov)), float(np.median(t_sg))
            out["workloads"].append({
                "name": "%s %s" % (shape, "with CIGAR" if cigar else "score only"), "timing": how,
                "entry": "EndsFreePlan" if plans else entry, "len_q": lq, "len_db": ld, "pairs": n,
                "overlap_ms": round(med_ov, 3), "overlap_gcups": round(cells / med_ov / 1e6, 1),
                "overlap_ms_min_max": [round(min(t_ov), 3), round(max(t_ov), 3)],
                "semi_global_ms": round(med_sg, 3), "semi_global_gcups": round(cells / med_sg / 1e6, 1),
                "semi_global_ms_min_max": [round(min(t_sg), 3), round(max(t_sg), 3)],
                "overlap_median_inside_semi_global_range": bool(min(t_sg) <= med_ov <= max(t_sg)),
                "ratio_overlap_over_semi_global": round(med_sg / med_ov, 3),
                "overlap_ms_samples": [round(t, 3) for t in t_ov],
                "semi_global_ms_samples": [round(t, 3) for t in t_sg],
                "model_check": {"pairs": k, "ok": ok},
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
