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
every workload is checked against tests/overlap_model.py.  Prints one JSON
line and writes it, with every sample, to --out (default
profiles/overlap_bench.json).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEMI_GLOBAL, OVERLAP = 2, 4


def _events_ms(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _wall_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _short_pairs(synth, distinct, lq=150, ld=400):
    """bench_ends_free.py's 150 x 400 pairs: the read's mutated copy inside a random window."""
    seed = 0x5EED0E0F
    allq = synth.random_bases(seed, distinct * lq).tobytes()
    pad = synth.random_bases(seed ^ 0xDB, distinct * ld).tobytes()
    qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
    ds = []
    for k, q in enumerate(qs):
        w = bytearray(pad[k * ld:(k + 1) * ld])
        m = synth.mutate(q, 0.05, seed=k)[:ld]
        at = (k * 37) % (ld - len(m) + 1)
        w[at:at + len(m)] = m
        ds.append(bytes(w))
    return qs, ds


def _long_pairs(synth, distinct, lq=2048, ld=2000):
    """bench_ends_free_long.py's 2,048 x 2,000 pairs: the query's mutated middle inside a window."""
    seed = 0x5EED10F6
    allq = synth.random_bases(seed, distinct * lq).tobytes()
    pad = synth.random_bases(seed ^ 0xDB, distinct * ld).tobytes()
    qs = [allq[k * lq:(k + 1) * lq] for k in range(distinct)]
    ds = []
    for k, q in enumerate(qs):
        w = bytearray(pad[k * ld:(k + 1) * ld])
        m = synth.mutate(q[200:1800], 0.05, seed=k)[:1600]
        w[200:200 + len(m)] = m
        ds.append(bytes(w))
    return qs, ds


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
    from sequencealigning_amd import _lib, synth
    import overlap_model as model

    ef = saln.ends_free
    L = _lib.lib()
    ctx = _lib.context(0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = {"steps": a.steps, "warmup": a.warmup, "alternations": a.alternations,
           "device": torch.cuda.get_device_name(0), "yardstick": "semi-global, same call, same pairs",
           "workloads": []}
    shapes = (("150x400", _short_pairs(synth, a.distinct), a.pairs, "saln_ends_free_align_batch"),
              ("2048x2000", _long_pairs(synth, a.long_distinct), a.long_pairs,
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
                timer, how = _events_ms, "device resident, hipEvents"
            else:
                def batch(mode):
                    def call():
                        h = C.c_void_p()
                        _lib.check(getattr(L, entry)(
                            ctx, vp(q_seq), vp(q_off), len(q_off) - 1, vp(d_seq), vp(d_off),
                            len(d_off) - 1, vp(idx), vp(idx), n, mode, None, 0, int(cigar),
                            C.byref(h)), entry)
                        L.saln_ends_free_aln_free(h)
                    return call
                run = {m: batch(m) for m in (OVERLAP, SEMI_GLOBAL)}
                timer = _wall_ms
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
            ok = True
            for j in range(k):
                m = model.align(qs[j], ds[j], walk=cigar)
                ok &= tuple(int(v) for v in got[j]) == m.record()
                ok &= cig.words(j).tolist() == model.cigar_words(m.cigar)
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
                "model_check": {"pairs": k, "ok": bool(ok)},
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
