"""CIGARs of long pairs under X-drop: the tiled replay
(saln_ends_free_xdrop_replay_align_batch, ends_free_xdrop_replay_kernels.hip)
against the full codes (saln_ends_free_xdrop_long_align_batch) on the same
pairs, in alternation in one process.

    python tools/bench_xdrop_replay.py [--pairs 3072] [--steps 10] [--warmup 2] [--alternations 2] [--out FILE]

Workloads (b) and (c) of bench_xdrop_long.py, with CIGARs, default scoring,
X = 100, the default trace budget of 1 GiB per chunk and the default tile rows:
  (b) 20,000 x 20,000, each db a 5 % mutated copy of its query: the band.
  (c) 20,000 x 20,000, the mutated copy in the first tenth of the db's rows,
      random bases after it: dead chunks.
Neither entry point has a device-resident form and both wait for their own
stream before they return, so the time is the wall clock of the C call (host
buffers in, records and words out), as in bench_xdrop_long.py.  What differs
between the two sides is what a pair holds against the trace budget (derived,
not measured: 200,000,000 bytes of codes against 12,830,528 of replay
footprint, 5 against 83 pairs per chunk) and how its words are found (one walk
over the codes against up to chunks + row blocks - 1 rounds of tile fill and
walk).  Every record (all fields but `reserved`) and the words of the first
--check pairs must be equal on both sides.  Prints one JSON line (and writes
it to --out).
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np

from ends_free_bench_util import wall_ms

SCORING = (5, -4, -8, -6)
SIDES = {"codes": "saln_ends_free_xdrop_long_align_batch", "replay": "saln_ends_free_xdrop_replay_align_batch"}


def call(entry, q_seq, q_off, d_seq, d_off, idx, X, keep, n_words):
    """One call of `entry` per run(); keep (a dict) receives the last run's
    records and the words of its first n_words pairs."""
    from sequencealigning_amd import _lib
    L, ctx = _lib.lib(), _lib.context(0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

    def run():
        h = C.c_void_p()
        _lib.check(getattr(L, entry)(
            ctx, vp(q_seq), vp(q_off), len(q_off) - 1, vp(d_seq), vp(d_off), len(d_off) - 1,
            vp(idx), vp(idx), len(idx), None, int(X), 0, 1, C.byref(h)), entry)
        if keep is not None:
            res = np.zeros(len(idx), dtype=_lib.ENDS_FREE_RESULT_DTYPE)
            r, cp, words = _lib.EndsFreeResult(), C.POINTER(C.c_uint32)(), []
            for k in range(len(idx)):
                L.saln_ends_free_aln_get(h, k, C.byref(r), C.byref(cp))
                res[k] = (r.score, r.status, r.q_begin, r.q_end, r.db_begin, r.db_end, r.cigar_len, r.reserved)
                if k < n_words:
                    words.append([cp[n] for n in range(r.cigar_len)])
            keep["res"], keep["words"] = res, words
        L.saln_ends_free_aln_free(h)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3072)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--check", type=int, default=16, help="pairs whose words are compared")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    R = _lib.get_option("ends_free.tile_rows")[0]
    out = {"pairs": a.pairs, "steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "scoring": list(SCORING), "tile_rows": R, "trace_budget_bytes": 1 << 30,
           "device": torch.cuda.get_device_name(0), "workloads": []}
    lq = ld = 20000
    X, distinct = 100, 64
    bytes_of = {"codes": ef.trace_bytes_long(lq, ld), "replay": ef.xdrop_replay_bytes(lq, ld, R)}
    for name, hom in (("b 20000x20000 the band, with codes", ld),
                      ("c 20000x20000 match ends after a tenth, with codes", ld // 10)):
        seed = 0x5EED0D21
        allq = synth.random_bases(seed, distinct * lq).tobytes()
        junk = synth.random_bases(seed ^ 0xDB, distinct * ld).tobytes()
        qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
        ds = [((synth.mutate(q, 0.05, seed=k) + q)[:hom] + junk[k * ld:(k + 1) * ld])[:ld] for k, q in enumerate(qs)]
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.ascontiguousarray(np.arange(a.pairs, dtype=np.uint32) % np.uint32(distinct))
        runs = {side: call(entry, q_seq, q_off, d_seq, d_off, idx, X, None, 0) for side, entry in SIDES.items()}
        ts = {side: [] for side in SIDES}
        for _ in range(a.alternations):
            for side in SIDES:
                ts[side] += wall_ms(runs[side], a.warmup, a.steps)
                print(name, side, [round(t, 1) for t in ts[side][-a.steps:]], "ms", file=sys.stderr, flush=True)
        # the records and words of one more, untimed call of each
        kept = {side: {} for side in SIDES}
        for side, entry in SIDES.items():
            call(entry, q_seq, q_off, d_seq, d_off, idx, X, kept[side], a.check)()
        got, ref = kept["replay"]["res"], kept["codes"]["res"]
        fields = ("score", "status", "q_begin", "q_end", "db_begin", "db_end", "cigar_len")
        ok = all(bool((got[f] == ref[f]).all()) for f in fields)
        ok &= bool((got["status"] == 0).all() and (got["cigar_len"] > 0).all())
        ok &= kept["replay"]["words"] == kept["codes"]["words"] and len(kept["codes"]["words"]) > 0
        med = {side: float(np.median(t)) for side, t in ts.items()}
        w = {"name": name, "len_q": lq, "len_db": ld, "homologous_rows": hom, "xdrop": X, "pairs": a.pairs,
             "samples_each": len(ts["codes"]),
             "replay_over_codes_time": round(med["replay"] / med["codes"], 4),
             "records_equal": bool(ok), "words_compared_pairs": len(kept["codes"]["words"]),
             "cigar_words_mean": round(float(ref["cigar_len"].mean()), 1)}
        for side in SIDES:
            w[side] = {"bytes_per_pair": bytes_of[side], "pairs_per_trace_chunk": (1 << 30) // bytes_of[side],
                       "trace_chunks": -(-a.pairs // ((1 << 30) // bytes_of[side])),
                       "ms": round(med[side], 3), "ms_min_max": [round(min(ts[side]), 3), round(max(ts[side]), 3)],
                       "reserved_mean": round(float(kept[side]["res"]["reserved"].mean()), 1),
                       "reserved_max": int(kept[side]["res"]["reserved"].max())}
        out["workloads"].append(w)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(w["records_equal"] for w in out["workloads"]):
        raise SystemExit("check failed")


if __name__ == "__main__":
    main()
