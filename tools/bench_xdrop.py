"""The X-drop extension (saln_ends_free_xdrop_plan_create) against plain
extension (SALN_MODE_EXTEND) on the same pairs, in alternation in one process.

    python tools/bench_xdrop.py [--steps 10] [--warmup 2] [--alternations 3]

Workloads (score only, EndsFreePlan, device resident, hipEvents):
  (a) nothing stops: each db a 5 % mutated copy of its query, X far above
      what any cell can drop.  What the extra instructions per cell cost.
        150 x 150      100,000 pairs
        1,000 x 1,000  25,000 pairs
  (b) the early stop: homology (the same mutated copy) in the first tenth of
      the db's rows, random bases after it, X = 100.  The time beside the ratio
      of the row-loop steps, read from the records' `reserved`, to the
      m + lanes - 1 steps of the plain fill.
        150 x 1,500     50,000 pairs
        1,000 x 10,000  5,000 pairs
A sample of every workload is checked against the models (tests/
ends_free_model.py, tests/xdrop_model.py), the steps against their bound.
Prints one JSON line.
"""
import argparse
import json

import numpy as np

from ends_free_bench_util import events_ms, model_check

EXTEND = 8
SCORING = (5, -4, -8, -6)
LARGE_X = 1 << 24


def xdrop_check(saln, got, qs, ds, X):
    """True when record k of `got` is xdrop_model's of qs[k] with ds[k] and
    its steps lie within their bound."""
    import xdrop_model
    ok = True
    for k in range(len(got)):
        a, _, L = xdrop_model.align(qs[k], ds[k], X, SCORING, walk=False)
        lanes = saln.ends_free.pair_geometry(len(qs[k]))[0]
        ok &= tuple(int(v) for v in got[k])[:7] == a.record()[:7]
        ok &= max(L, 1) <= int(got["reserved"][k]) <= xdrop_model.steps_bound(len(ds[k]), L, lanes)
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="factor on every workload's pairs")
    ap.add_argument("--check", type=int, default=2, help="pairs per workload and engine checked against the models")
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    out = {"steps": a.steps, "warmup": a.warmup, "alternations": a.alternations, "scoring": list(SCORING),
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, lq, ld, hom, X, n_pairs, distinct in (
            ("a 150x150 nothing stops", 150, 150, 150, LARGE_X, 100_000, 2_000),
            ("a 1000x1000 nothing stops", 1000, 1000, 1000, LARGE_X, 25_000, 500),
            ("b 150x1500 homology in the first tenth", 150, 1500, 150, 100, 50_000, 2_000),
            ("b 1000x10000 homology in the first tenth", 1000, 10000, 1000, 100, 5_000, 250)):
        n_pairs = max(64, int(n_pairs * a.scale))
        seed = 0x5EED0D20
        allq = synth.random_bases(seed, distinct * lq).tobytes()
        junk = synth.random_bases(seed ^ 0xDB, distinct * ld).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
        ds = [((synth.mutate(q, 0.05, seed=k) + q)[:hom] + junk[k * ld:(k + 1) * ld])[:ld] for k, q in enumerate(qs)]
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.arange(n_pairs, dtype=np.uint32) % np.uint32(distinct)
        pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
        dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
        dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
        runs, plans, outs = {}, [], {}
        for key, xdrop in (("extend", None), ("xdrop", X)):
            plan = ef.EndsFreePlan(q_off, d_off, pairs, mode=EXTEND, scoring=SCORING, xdrop=xdrop)
            res = torch.zeros(n_pairs * 8, dtype=torch.int32, device="cuda")
            runs[key] = lambda plan=plan, res=res: plan.execute(dq, dd, res)
            plans.append(plan)
            outs[key] = res
        ts = {"extend": [], "xdrop": []}
        for _ in range(a.alternations):
            for key in ("extend", "xdrop"):
                ts[key] += events_ms(runs[key], a.warmup, a.steps)
        torch.cuda.synchronize()
        got = {key: res.cpu().numpy().view(_lib.ENDS_FREE_RESULT_DTYPE) for key, res in outs.items()}
        for plan in plans:
            plan.close()
        lanes = ef.pair_geometry(lq)[0]
        steps = got["xdrop"]["reserved"].astype(np.float64)
        # a sample against the models: the timed runs' own records
        k = min(a.check, distinct)
        ok = model_check(got["extend"][:k], None, qs, ds, EXTEND, SCORING, False)
        ok &= xdrop_check(saln, got["xdrop"][:k], qs, ds, X)
        if X == LARGE_X:
            ok &= bool((got["xdrop"]["score"] == got["extend"]["score"]).all())
        med = {key: float(np.median(t)) for key, t in ts.items()}
        cells = float(lq) * ld * n_pairs
        out["workloads"].append({
            "name": name, "len_q": lq, "len_db": ld, "homologous_rows": hom, "xdrop": X, "pairs": n_pairs,
            "extend_ms": round(med["extend"], 3),
            "extend_ms_min_max": [round(min(ts["extend"]), 3), round(max(ts["extend"]), 3)],
            "xdrop_ms": round(med["xdrop"], 3),
            "xdrop_ms_min_max": [round(min(ts["xdrop"]), 3), round(max(ts["xdrop"]), 3)],
            "xdrop_over_extend_time": round(med["xdrop"] / med["extend"], 4),
            "extend_gcups": round(cells / med["extend"] / 1e6, 1),
            "steps_mean": round(float(steps.mean()), 1), "steps_max": int(steps.max()),
            "plain_steps": ld + lanes - 1,
            "step_ratio": round(float(steps.mean()) / (ld + lanes - 1), 4),
            "samples_each": len(ts["extend"]), "model_check": {"pairs": k, "ok": bool(ok)},
        })
    print(json.dumps(out))
    if not all(w["model_check"]["ok"] for w in out["workloads"]):
        raise SystemExit("model check failed")


if __name__ == "__main__":
    main()
