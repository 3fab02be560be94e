"""configs[2] (C3) shape with the *corrected* gap-affine WFA engine
(not reference parity): minimum penalty (x=4, o=2,
e=6, src/wfa.rs:14-21) of 10 kbp G-mut(5%) pairs through the device-resident
plan (sequences and scores in HBM).  n_pairs pairs drawn over `distinct`
generated pairs (pair k uses pair k % distinct).  A seeded sample of the
distinct pairs is checked against the Gotoh DP (oracle/refaffine.c, test
infrastructure), which is also timed on the host as the CPU baseline.

    python tools/bench_wfa_affine.py [--pairs 100000] [--distinct 2000] [--reps 2] [--align]

--align: the same pairs also go through wfa_affine_align_batch (host buffers
in, CIGARs out: score passes, trace fill and walk in chunks of --budget bytes
of trace codes); its pairs/s is printed next to the score-only figure of the
same run, with the trace bytes per pair, and a sample of CIGARs is checked
(consumes both sequences, penalty = score).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=2_000)
    ap.add_argument("--len", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--check", type=int, default=4, help="pairs checked against the DP oracle")
    ap.add_argument("--align", action="store_true", help="also time wfa_affine_align_batch")
    ap.add_argument("--budget", type=int, default=0, help="--align: trace bytes per chunk (0: 1 GiB)")
    a = ap.parse_args()
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import synth
    seed = 0x5EED0003
    allq = synth.random_bases(seed, a.distinct * a.len).tobytes()
    qs = [allq[k * a.len:(k + 1) * a.len] for k in range(a.distinct)]
    ds = [synth.mutate(q, 0.05, seed=k) for k, q in enumerate(qs)]
    q_seq, q_off = saln.pack_csr(qs)
    d_seq, d_off = saln.pack_csr(ds)
    k = np.arange(a.pairs, dtype=np.uint32) % np.uint32(a.distinct)
    plan = saln.wfa_affine.WfaAffinePlan(q_off, d_off, np.stack([k, k], 1))
    dq = torch.from_numpy(q_seq.copy()).cuda()
    dd = torch.from_numpy(d_seq.copy()).cuda()
    sc = torch.zeros(a.pairs, dtype=torch.int32, device="cuda")
    plan.execute(dq, dd, sc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        plan.execute(dq, dd, sc)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.reps
    s = sc.cpu().numpy()
    from oracle import refcpu  # checker only
    t0 = time.perf_counter()
    chk = [(j, int(s[j]), refcpu.affine_penalty(qs[j], ds[j]))
           for j in range(min(a.check, a.distinct))]
    cpu_s = (time.perf_counter() - t0) / max(1, len(chk))
    ok = all(g == w for _, g, w in chk)
    cells = float(a.len) * a.len * a.pairs
    align = None
    if a.align:
        wa = saln.wfa_affine
        pairs = np.stack([k, k], 1)
        t0 = time.perf_counter()
        res, cig = wa.wfa_affine_align_batch(qs, ds, pairs, trace_budget=a.budget)
        adt = time.perf_counter() - t0
        tb = [wa.trace_bytes(len(qs[j]), len(ds[j]), int(s[j])) for j in range(a.distinct)
              if s[j] >= 0]
        good = True
        for j in range(0, a.pairs, max(1, a.pairs // 64)):
            c = cig[j]
            jq, jd = qs[int(k[j])], ds[int(k[j])]
            good &= int(res["status"][j]) == 0 and int(res["score"][j]) == int(s[j])
            good &= wa.cigar_penalty(c) == int(s[j])
            good &= sum(n for n, op in c if op in "=XI") == len(jq)
            good &= sum(n for n, op in c if op in "=XD") == len(jd)
        align = {"ms": round(adt * 1e3, 1), "pairs_per_s": round(a.pairs / adt, 1),
                 "score_only_pairs_per_s": round(a.pairs / dt, 1),
                 "trace_bytes_per_pair": round(float(np.mean(tb)), 1) if tb else None,
                 "cigar_words_per_pair": round(float(res["cigar_len"].mean()), 1),
                 "status_ok": int((res["status"] == 0).sum()), "sample_ok": bool(good),
                 "note": "host buffers in, CIGARs out (score passes + trace fill + walk + copies)"}
    print(json.dumps({
        "workload": f"configs[2] shape, corrected gap-affine WFA (score only): {a.pairs} pairs "
                    f"({a.distinct} distinct) of {a.len} bp G-mut(5%)",
        "pairs": a.pairs, "ms": round(dt * 1e3, 3), "pairs_per_s": round(a.pairs / dt, 1),
        "equiv_gcups": round(cells / dt / 1e9, 1),
        "penalty_mean": float(np.mean(s[s >= 0])) if (s >= 0).any() else None,
        "over_width": int((s == -2).sum()), "over_cap": int((s == -1).sum()),
        "dp_check": {"pairs": len(chk), "ok": ok, "sample": chk[:4]},
        "cpu_baseline": {"kind": "oracle Gotoh DP (O(n*m), not a WFA)", "cores": 1,
                         "s_per_pair": round(cpu_s, 3), "pairs_per_s": round(1 / cpu_s, 3)},
        **({"align": align} if align else {}),
    }))
    plan.close()


if __name__ == "__main__":
    main()
