"""The tiled replay traceback (saln_ends_free_replay_align_batch,
ends_free_replay_kernels.hip) next to the long entry point with its full trace
(saln_ends_free_long_align_batch), on the same pairs.

    python tools/bench_ends_free_replay.py [--tile-rows 0] [--workloads 0,1,2,3]
                                           [--steps 10] [--warmup 2] [--alternations 3]

Workloads, all with CIGAR, the default trace budget (1 GiB per chunk) on both
sides, G-mut(5%) pairs:
  0  512 local pairs of 2,048 x 2,000
  1  16 local pairs of 20,000 x 20,000   (the full trace: 200 MB a pair)
  2  one lone local 20,000 x 20,000 pair
  3  32 semi-global pairs of 5,000 x 100,000: a read against a window (250 MB a pair)
Timing: the wall clock of the C call, host buffers in, handle out.  Protocol:
replay and the long entry point in one process in alternation, `alternations`
x (`warmup` + `steps`); a workload whose first call takes more than a second
runs alternations x (1 + 2) instead, and its entry says so ("steps",
"warmup").  Every workload's sample of pairs (--check) is run through both
entry points by the Python interface and compared, record and words.  Prints
one JSON line and writes it, with every sample, to --out (default
profiles/ends_free_replay_bench.json).  --tile-rows 0: the option's default.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from ends_free_bench_util import ROOT, batch_call, wall_ms


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3),
            "max_ms": round(max(ts), 3), "samples_ms": [round(t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile-rows", type=int, default=0)
    ap.add_argument("--workloads", default="0,1,2,3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--check", type=int, default=2, help="pairs per workload compared with the long entry point")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_free_replay_bench.json"))
    a = ap.parse_args()
    import torch
    import sequencealigning_amd as saln
    from sequencealigning_amd import _lib, synth

    ef = saln.ends_free
    if a.tile_rows:
        _lib.set_option("ends_free.tile_rows", a.tile_rows)
    R = _lib.get_option("ends_free.tile_rows")[0]
    seed = 0x5EED7113

    def square(n, count, s):
        qs, ds = [], []
        for k in range(count):
            q = synth.random_bases(s + 2 * k, n).tobytes()
            d = synth.mutate(q, 0.05, seed=s + 2 * k + 1)
            qs.append(q)
            ds.append((d + synth.random_bases(s ^ (k + 0x99), n).tobytes())[:n])
        return qs, ds

    def windows(n, m, count, s):
        qs, ds = [], []
        for k in range(count):
            d = synth.random_bases(s + 2 * k, m).tobytes()
            lo = (k * 2671 + 500) % (m - n - 100)
            qs.append(synth.mutate(d[lo:lo + n], 0.05, seed=s + 2 * k + 1)[:n])
            ds.append(d)
        return qs, ds

    def wide(count):   # 2,048 x 2,000: the query's mutated middle inside a random window
        qs, ds = [], []
        for k in range(count):
            q = synth.random_bases(seed + 3 * k, 2048).tobytes()
            w = bytearray(synth.random_bases(seed + 3 * k + 1, 2000).tobytes())
            m = synth.mutate(q[200:1800], 0.05, seed=k)[:1600]
            w[200:200 + len(m)] = m
            qs.append(q)
            ds.append(bytes(w))
        return qs, ds

    specs = [
        ("512 local pairs 2048x2000", 1, lambda: wide(512)),
        ("16 local pairs 20000x20000", 1, lambda: square(20000, 16, seed ^ 0x16)),
        ("lone local pair 20000x20000", 1, lambda: square(20000, 1, seed ^ 0x10E)),
        ("32 semi-global pairs 5000x100000", 2, lambda: windows(5000, 100000, 32, seed ^ 0x32)),
    ]
    out = {"tile_rows": R, "alternations": a.alternations, "device": torch.cuda.get_device_name(0),
           "timing": "host buffers in, handle out, wall clock of the C call", "workloads": []}
    for w in (int(x) for x in a.workloads.split(",")):
        name, mode, make = specs[w]
        qs, ds = make()
        n = len(qs)
        q_seq, q_off = saln.pack_csr(qs)
        d_seq, d_off = saln.pack_csr(ds)
        idx = np.arange(n, dtype=np.uint32)

        run_replay, run_long = (batch_call(entry, q_seq, q_off, d_seq, d_off, idx, idx, mode, None, 1)
                                for entry in ("saln_ends_free_replay_align_batch", "saln_ends_free_long_align_batch"))
        t0 = time.perf_counter()
        run_long()
        slow = time.perf_counter() - t0 > 1.0
        warmup, steps = (1, 2) if slow else (a.warmup, a.steps)
        t_replay, t_long = [], []
        for _ in range(a.alternations):
            t_replay += wall_ms(run_replay, warmup, steps)
            t_long += wall_ms(run_long, warmup, steps)
        k = min(a.check, n)
        pairs = [(j, j) for j in range(k)]
        got, gcig = ef.ends_free_align_long_batch(qs[:k], ds[:k], pairs, mode=mode, replay=True)
        ref, rcig = ef.ends_free_align_long_batch(qs[:k], ds[:k], pairs, mode=mode)
        ok = bool((got == ref).all()) and all(gcig.words(j).tolist() == rcig.words(j).tolist() for j in range(k))
        ok = ok and all(int(got["status"][j]) == 0 and int(got["cigar_len"][j]) > 0 for j in range(k))
        cells = float(sum(len(q) * len(d) for q, d in zip(qs, ds)))
        sr, sl = _stats(t_replay), _stats(t_long)
        out["workloads"].append({
            "name": name, "pairs": n, "len_q": len(qs[0]), "len_db": len(ds[0]), "steps": steps, "warmup": warmup,
            "replay_bytes_per_pair": ef.replay_bytes(len(qs[0]), len(ds[0]), R),
            "trace_bytes_per_pair": ef.trace_bytes_long(len(qs[0]), len(ds[0])),
            "replay": sr, "long": sl,
            "replay_gcups": round(cells / sr["median_ms"] / 1e6, 1),
            "long_gcups": round(cells / sl["median_ms"] / 1e6, 1),
            "speedup_replay_over_long": round(sl["median_ms"] / sr["median_ms"], 3),
            "check": {"pairs": k, "ok": ok},
        })
        print(json.dumps(out["workloads"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(w["check"]["ok"] for w in out["workloads"]):
        raise SystemExit("replay differs from the long entry point")


if __name__ == "__main__":
    main()
