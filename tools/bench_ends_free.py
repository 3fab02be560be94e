"""Throughput of the ends-free engine (local / semi-global; not reference
parity) next to the project's own global i32 lane fill on the same shapes.

    python tools/bench_ends_free.py [--pairs 100000] [--steps 10] [--warmup 2] [--alternations 3]

Workloads (G-mut(5%) pairs, `distinct` generated pairs drawn round-robin):
  local 150x150 score only       EndsFreePlan, device resident, hipEvents
  local 150x150 with CIGAR       saln_ends_free_align_batch, host buffers in, CIGARs out (wall)
  semi-global 150x400 with CIGAR the same
Yardstick, measured in the same process in alternation with each workload:
an NwPlan (global) over the same pairs under a scheme whose pairs
saln_nw_plan_pair_path reports as packed = 0 (the i32 lane fill): score only
(device resident, hipEvents) and saln_nw_align_batch (host buffers in, CIGARs
out, wall) for the CIGAR workloads.  GCUPS = len_q * len_db * pairs / time.
A sample of every workload is checked against tests/ends_free_model.py.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json

import numpy as np

from ends_free_bench_util import batch_call, events_ms, model_check, short_pairs, wall_ms


def _i32_scheme(saln, q_off, d_off, pairs):
    """The first multiple of the default scheme the NW plan runs on i32 lanes."""
    for k in (1, 4, 16, 64, 256, 1024, 4096):
        sc = (5 * k, -4 * k, -8 * k, -6 * k)
        plan = saln.NwPlan(q_off, d_off, pairs[:64], scoring=sc)
        packed = plan.pair_path(0).packed
        plan.close()
        if not packed:
            return sc
    raise SystemExit("no scheme found that the NW plan runs on i32 lanes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=2_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=24, help="pairs per workload checked against the model")
    a = ap.parse_args()
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    L = _lib.lib()
    out = {"pairs": a.pairs, "steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, mode, lq, ld, cigar in (("local 150x150 score only", 1, 150, 150, False),
                                      ("local 150x150 with CIGAR", 1, 150, 150, True),
                                      ("semi-global 150x400 with CIGAR", 2, 150, 400, True)):
        seed = 0x5EED0E0F
        allq = synth.random_bases(seed, a.distinct * lq).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(a.distinct)]
        if ld == lq:
            ds = [(synth.mutate(q, 0.05, seed=k) + q)[:ld] for k, q in enumerate(qs)]
        else:
            qs, ds = short_pairs(synth, a.distinct, seed, lq, ld)
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.arange(a.pairs, dtype=np.uint32) % np.uint32(a.distinct)
        pairs = np.ascontiguousarray(np.stack([idx, idx], 1))
        cells = float(lq) * ld * a.pairs
        sc_i32 = _i32_scheme(saln, q_off, d_off, pairs)
        dq = torch.from_numpy(np.concatenate([q_seq, np.zeros(16, np.uint8)])).cuda()
        dd = torch.from_numpy(np.concatenate([d_seq, np.zeros(16, np.uint8)])).cuda()
        nw_plan = saln.NwPlan(q_off, d_off, pairs, scoring=sc_i32)
        assert not nw_plan.pair_path(0).packed
        nw_res = torch.zeros(a.pairs * 4, dtype=torch.int32, device="cuda")
        if not cigar:
            nw_plan.set_score_only(True)
            plan = ef.EndsFreePlan(q_off, d_off, pairs, mode=mode)
            res = torch.zeros(a.pairs * 8, dtype=torch.int32, device="cuda")
            run_ef = lambda: plan.execute(dq, dd, res)                 # noqa: E731
            run_nw = lambda: nw_plan.execute(dq, dd, nw_res)           # noqa: E731
            timer, how = events_ms, "device resident, hipEvents"
        else:
            vp = lambda x: x.ctypes.data_as(C.c_void_p)                # noqa: E731
            pq, pd = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            ctx = _lib.context(0)
            run_ef = batch_call("saln_ends_free_align_batch", q_seq, q_off, d_seq, d_off, pq, pd, mode, None, 1)
            nw_out = np.zeros(a.pairs, dtype=_lib.RESULT_DTYPE)
            coff = np.arange(a.pairs + 1, dtype=np.uint64) * np.uint64(lq + ld)
            nw_cig = np.zeros(int(coff[-1]), np.uint32)
            sarg = _lib.scoring_arg(sc_i32)

            def run_nw():
                _lib.check(L.saln_nw_align_batch(
                    ctx, vp(q_seq), vp(q_off), len(q_off) - 1, vp(d_seq), vp(d_off), len(d_off) - 1,
                    vp(pq), vp(pd), a.pairs, 0, sarg, vp(nw_out), vp(nw_cig), vp(coff)),
                    "nw_align_batch")

            timer, how = wall_ms, "host buffers in, CIGARs out, wall clock of the C call"
        t_ef, t_nw = [], []
        for _ in range(a.alternations):
            t_ef += timer(run_ef, a.warmup, a.steps)
            t_nw += timer(run_nw, a.warmup, a.steps)
        # a sample against the model
        k = min(a.check, a.distinct)
        got, cig = ef.ends_free_align_batch(qs[:k], ds[:k], [(j, j) for j in range(k)], mode=mode,
                                            cigar=cigar)
        ok = model_check(got, cig, qs, ds, mode, None, cigar)
        med_ef, med_nw = float(np.median(t_ef)), float(np.median(t_nw))
        out["workloads"].append({
            "name": name, "timing": how, "len_q": lq, "len_db": ld,
            "ends_free_ms": round(med_ef, 3), "ends_free_gcups": round(cells / med_ef / 1e6, 1),
            "ends_free_ms_min_max": [round(min(t_ef), 3), round(max(t_ef), 3)],
            "nw_i32_scheme": list(sc_i32),
            "nw_i32_ms": round(med_nw, 3), "nw_i32_gcups": round(cells / med_nw / 1e6, 1),
            "nw_i32_ms_min_max": [round(min(t_nw), 3), round(max(t_nw), 3)],
            "ratio_ends_free_over_nw": round(med_nw / med_ef, 3),
            "samples_each": len(t_ef), "model_check": {"pairs": k, "ok": ok},
        })
        nw_plan.close()
        if not cigar:
            plan.close()
    print(json.dumps(out))
    if not all(w["model_check"]["ok"] for w in out["workloads"]):
        raise SystemExit("model check failed")


if __name__ == "__main__":
    main()
