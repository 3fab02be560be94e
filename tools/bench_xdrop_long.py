"""The chunked X-drop fill (saln_ends_free_xdrop_long_align_batch,
ends_free_xdrop_long_kernels.hip) against plain extension on the long path
(saln_ends_free_long_align_batch, SALN_MODE_EXTEND) on the same pairs, in
alternation in one process.

    python tools/bench_xdrop_long.py [--steps 10] [--warmup 2] [--alternations 3] [--out FILE]
    python tools/bench_xdrop_long.py --merge RUN1.json RUN2.json RUN3.json --out profiles/ends_free_xdrop_long_bench.json

Neither entry point has a device-resident form, and both wait for their own
stream before they return, so the time is the wall clock of the C call (host
buffers in, records out), as in bench_ends_free_long.py: uploads and
allocations are the same on both sides.  Default scoring; every workload score
only and with codes (CIGARs):
  (a) 2,048 x 2,000, each db a 5 % mutated copy of its query, X far above what
      any cell can drop: nothing is pruned.  The price of the rule on the
      chunked fill.  At 4,096 pairs and at the 3,072 of (b) and (c).
  (b) 20,000 x 20,000, 5 % mutated, X = 100: the band.
  (c) 20,000 x 20,000, the mutated copy in the first tenth of the db's rows,
      random bases after it, X = 100: dead chunks.
The records' `reserved` gives the row-loop steps; the plain fill runs
chunks x (m + 63).  A sample is checked against the schedule
model (tests/xdrop_long_model.py, which test_xdrop_long_model.py holds to the
plain model), the steps against their bound; a sample of (c) only: (b)'s
windows hold some 20 million cells.  In (a) every score and end must equal plain
extension's, in (b) and (c) none may lie above it.  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import json

import numpy as np

from ends_free_bench_util import wall_ms

EXTEND = 8
SCORING = (5, -4, -8, -6)
LARGE_X = 1 << 24


def call(entry, q_seq, q_off, d_seq, d_off, idx, mode_or_x, want_cigar, keep):
    """One call of `entry` per run(); keep["res"] holds the last run's records."""
    from sequencealigning_amd import _lib
    L, ctx = _lib.lib(), _lib.context(0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    xdrop = "xdrop" in entry
    args = (None, int(mode_or_x)) if xdrop else (int(mode_or_x), None)

    def run():
        h = C.c_void_p()
        _lib.check(getattr(L, entry)(
            ctx, vp(q_seq), vp(q_off), len(q_off) - 1, vp(d_seq), vp(d_off), len(d_off) - 1,
            vp(idx), vp(idx), len(idx), *args, 0, int(want_cigar), C.byref(h)), entry)
        if keep is not None:
            res = np.zeros(len(idx), dtype=_lib.ENDS_FREE_RESULT_DTYPE)
            r = _lib.EndsFreeResult()
            for k in range(len(idx)):
                L.saln_ends_free_aln_get(h, k, C.byref(r), None)
                res[k] = (r.score, r.status, r.q_begin, r.q_end, r.db_begin, r.db_end, r.cigar_len, r.reserved)
            keep["res"] = res
        L.saln_ends_free_aln_free(h)
    return run


def schedule_check(got, qs, ds, X, cigar):
    """True when record k is the schedule model's and its steps lie within the bound."""
    import xdrop_long_model as lm
    ok = True
    for k in range(len(got)):
        a, _, _, windows, bound = lm.align(qs[k], ds[k], X, SCORING, walk=cigar)
        want = a.record()[:6] if a.score else ((0, 0, 0, 0, 0, 0) if cigar else (0, 0, -1, 0, -1, 0))
        ok &= tuple(int(v) for v in got[k])[:6] == want
        ok &= 1 <= int(got["reserved"][k]) <= bound
    return bool(ok)


def merge(files, out_path):
    runs = [json.loads(open(f).readline()) for f in files]
    out = {"device": runs[0]["device"], "scoring": runs[0]["scoring"],
           "protocol": f"tools/bench_xdrop_long.py, {len(runs)} processes one after the other; each figure the median "
                       f"of {runs[0]['alternations']} x ({runs[0]['warmup']} warm-up + {runs[0]['steps']} timed) of one "
                       "process, plain long extension and the chunked X-drop fill in alternation; wall clock of "
                       "the C call, host buffers in, records out; ms",
           "workloads": {}}
    for i, w in enumerate(runs[0]["workloads"]):
        ws = [r["workloads"][i] for r in runs]
        assert all(x["name"] == w["name"] for x in ws)
        m = {k: w[k] for k in ("len_q", "len_db", "homologous_rows", "xdrop", "pairs", "codes", "chunks",
                               "plain_steps", "steps_mean", "steps_max", "step_ratio")}
        for key in ("extend_ms", "xdrop_ms", "xdrop_over_extend_time"):
            m[key] = [x[key] for x in ws]
        for key in ("extend_ms_min_max", "xdrop_ms_min_max"):
            m[key + "_of_all_samples"] = [min(x[key][0] for x in ws), max(x[key][1] for x in ws)]
        m["median_of_processes"] = {key: float(np.median(m[key])) for key in ("extend_ms", "xdrop_ms",
                                                                              "xdrop_over_extend_time")}
        m["check_ok"] = all(x["check"]["ok"] for x in ws)
        out["workloads"][w["name"]] = m
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="factor on every workload's pairs")
    ap.add_argument("--check", type=int, default=1, help="pairs per workload checked against the schedule model")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", nargs="+", help="merge these runs' JSON lines into --out")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    assert a.steps >= 10, "at least 10 timed steps"
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import synth

    out = {"steps": a.steps, "warmup": a.warmup, "alternations": a.alternations, "scoring": list(SCORING),
           "device": torch.cuda.get_device_name(0), "workloads": []}
    for name, lq, ld, hom, X, pairs_fill, pairs_codes, distinct in (
            ("a 2048x2000 nothing pruned, 4096 pairs", 2048, 2000, 2000, LARGE_X, 4096, 256, 256),
            ("a 2048x2000 nothing pruned, 3072 pairs", 2048, 2000, 2000, LARGE_X, 3072, 0, 256),
            ("b 20000x20000 the band", 20000, 20000, 20000, 100, 3072, 4, 64),
            ("c 20000x20000 match ends after a tenth", 20000, 20000, 2000, 100, 3072, 4, 64)):
        seed = 0x5EED0D21
        allq = synth.random_bases(seed, distinct * lq).tobytes()
        junk = synth.random_bases(seed ^ 0xDB, distinct * ld).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
        ds = [((synth.mutate(q, 0.05, seed=k) + q)[:hom] + junk[k * ld:(k + 1) * ld])[:ld] for k, q in enumerate(qs)]
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        chunks = saln.ends_free.pair_path_long(lq, ld)[1]
        for codes, n_pairs in ((0, pairs_fill), (1, pairs_codes)):
            if not n_pairs:
                continue
            n_pairs = max(4, int(n_pairs * a.scale))
            idx = np.ascontiguousarray(np.arange(n_pairs, dtype=np.uint32) % np.uint32(distinct))
            kept = {"extend": {}, "xdrop": {}}
            runs = {"extend": call("saln_ends_free_long_align_batch", q_seq, q_off, d_seq, d_off, idx, EXTEND, codes, None),
                    "xdrop": call("saln_ends_free_xdrop_long_align_batch", q_seq, q_off, d_seq, d_off, idx, X, codes, None)}
            ts = {"extend": [], "xdrop": []}
            for _ in range(a.alternations):
                for key in ("extend", "xdrop"):
                    ts[key] += wall_ms(runs[key], a.warmup, a.steps)
            # the records of one more, untimed call of each
            call("saln_ends_free_long_align_batch", q_seq, q_off, d_seq, d_off, idx, EXTEND, codes, kept["extend"])()
            call("saln_ends_free_xdrop_long_align_batch", q_seq, q_off, d_seq, d_off, idx, X, codes, kept["xdrop"])()
            got, plain = kept["xdrop"]["res"], kept["extend"]["res"]
            k = min(a.check, distinct, n_pairs)
            if X == LARGE_X:
                ok = bool((got["score"] == plain["score"]).all() and (got["q_end"] == plain["q_end"]).all()
                          and (got["db_end"] == plain["db_end"]).all() and (got["cigar_len"] == plain["cigar_len"]).all())
            else:
                # (b)'s windows hold some 20 million cells, too many for the model; (c)'s two million
                ok = schedule_check(got[:k], qs, ds, X, bool(codes)) if hom < ld else True
                ok &= bool((got["score"] <= plain["score"]).all() and (got["reserved"] >= 1).all())
            steps = got["reserved"].astype(np.float64)
            med = {key: float(np.median(t)) for key, t in ts.items()}
            plain_steps = chunks * (ld + 63)
            out["workloads"].append({
                "name": name + (", with codes" if codes else ", score only"), "len_q": lq, "len_db": ld,
                "homologous_rows": hom, "xdrop": X, "pairs": n_pairs, "codes": bool(codes), "chunks": chunks,
                "extend_ms": round(med["extend"], 3),
                "extend_ms_min_max": [round(min(ts["extend"]), 3), round(max(ts["extend"]), 3)],
                "xdrop_ms": round(med["xdrop"], 3),
                "xdrop_ms_min_max": [round(min(ts["xdrop"]), 3), round(max(ts["xdrop"]), 3)],
                "xdrop_over_extend_time": round(med["xdrop"] / med["extend"], 4),
                "steps_mean": round(float(steps.mean()), 1), "steps_max": int(steps.max()),
                "plain_steps": plain_steps, "step_ratio": round(float(steps.mean()) / plain_steps, 4),
                "samples_each": len(ts["extend"]),
                "records_equal_plain_extension": round(float((got["score"] == plain["score"]).mean()), 4),
                "check": {"pairs": k, "ok": bool(ok)},
            })
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(w["check"]["ok"] for w in out["workloads"]):
        raise SystemExit("check failed")


if __name__ == "__main__":
    main()
