"""Extension alignment (SALN_MODE_EXTEND) against local on the same pairs, in
alternation in one process: what the mode costs next to the mode whose work
it does without the floor and the stop code.

    python tools/bench_extend.py [--steps 10] [--warmup 2] [--alternations 3]

Workloads (score only; each db is a 5 % mutated copy of its query from the
first byte on, so that the extension runs the pair's length):
  150 x 150      100,000 pairs, EndsFreePlan, device resident, hipEvents
  1,000 x 1,000  25,000 pairs, the same
  2,048 x 2,000  4,096 pairs, the chunked fill (saln_ends_free_long_align_batch,
                 host buffers in, records out, wall clock of the C call)
A sample of every workload and mode is checked against the model
(tests/ends_free_model.py).  Prints one JSON line.
"""
import argparse
import json

import numpy as np

from ends_free_bench_util import batch_call, events_ms, model_check, wall_ms

LOCAL, EXTEND = 1, 8
SCORING = (5, -4, -8, -6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="factor on every workload's pairs")
    ap.add_argument("--check", type=int, default=6, help="pairs per workload and mode checked against the model")
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    out = {"steps": a.steps, "warmup": a.warmup, "alternations": a.alternations, "scoring": list(SCORING),
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, lq, ld, n_pairs, distinct, chunked in (("150x150 score only", 150, 150, 100_000, 2_000, False),
                                                    ("1000x1000 score only", 1000, 1000, 25_000, 500, False),
                                                    ("chunked 2048x2000 score only", 2048, 2000, 4_096, 256, True)):
        n_pairs = max(64, int(n_pairs * a.scale))
        seed = 0x5EED0E08
        allq = synth.random_bases(seed, distinct * lq).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
        ds = [(synth.mutate(q, 0.05, seed=k) + q)[:ld] for k, q in enumerate(qs)]
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.arange(n_pairs, dtype=np.uint32) % np.uint32(distinct)
        pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
        cells = float(lq) * ld * n_pairs
        assert ef.pair_path_long(lq, ld)[0] == int(chunked)
        runs, plans = {}, []
        if not chunked:
            dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
            dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
            for mode in (LOCAL, EXTEND):
                plan = ef.EndsFreePlan(q_off, d_off, pairs, mode=mode, scoring=SCORING)
                res = torch.zeros(n_pairs * 8, dtype=torch.int32, device="cuda")
                runs[mode] = lambda plan=plan, res=res: plan.execute(dq, dd, res)
                plans.append(plan)
            timer, how = events_ms, "EndsFreePlan, device resident, hipEvents"
        else:
            runs = {mode: batch_call("saln_ends_free_long_align_batch", q_seq, q_off, d_seq, d_off, idx, idx,
                                     mode, _lib.scoring_arg(SCORING), 0) for mode in (LOCAL, EXTEND)}
            timer, how = wall_ms, "host buffers in, records out, wall clock of the C call"
        ts = {LOCAL: [], EXTEND: []}
        for _ in range(a.alternations):
            for mode in (LOCAL, EXTEND):
                ts[mode] += timer(runs[mode], a.warmup, a.steps)
        for plan in plans:
            plan.close()
        # a sample against the model
        k = min(a.check, distinct)
        ok = True
        for mode in (LOCAL, EXTEND):
            got, _ = ef.ends_free_align_long_batch(qs[:k], ds[:k], [(j, j) for j in range(k)], mode=mode,
                                                   scoring=SCORING, cigar=False)
            ok &= model_check(got, None, qs, ds, mode, SCORING, False)
        med = {mode: float(np.median(t)) for mode, t in ts.items()}
        out["workloads"].append({
            "name": name, "timing": how, "len_q": lq, "len_db": ld, "pairs": n_pairs,
            "local_ms": round(med[LOCAL], 3), "local_ms_min_max": [round(min(ts[LOCAL]), 3), round(max(ts[LOCAL]), 3)],
            "extend_ms": round(med[EXTEND], 3),
            "extend_ms_min_max": [round(min(ts[EXTEND]), 3), round(max(ts[EXTEND]), 3)],
            "local_gcups": round(cells / med[LOCAL] / 1e6, 1), "extend_gcups": round(cells / med[EXTEND] / 1e6, 1),
            "extend_over_local_time": round(med[EXTEND] / med[LOCAL], 4),
            "samples_each": len(ts[LOCAL]), "model_check": {"pairs": k, "ok": ok},
        })
    print(json.dumps(out))
    if not all(w["model_check"]["ok"] for w in out["workloads"]):
        raise SystemExit("model check failed")


if __name__ == "__main__":
    main()
