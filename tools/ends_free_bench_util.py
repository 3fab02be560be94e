"""What the ends-free bench tools share (bench_ends_free.py, _long, _replay,
_sub, bench_overlap.py, bench_extend.py, bench_xdrop.py): the two timers, the two pair
generators, the raw C batch call and the sample check against the plain model
tests/ends_free_model.py.  Importing it puts the repository and tests/ on the
path."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def events_ms(fn, warmup, steps):
    """Device time of each of `steps` calls, by hipEvents."""
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


def wall_ms(fn, warmup, steps):
    """Wall clock of each of `steps` calls."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def short_pairs(synth, distinct, seed=0x5EED0E0F, lq=150, ld=400):
    """150 x 400 G-mut(5%) pairs: the read's mutated copy inside a random window."""
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


def long_pairs(synth, distinct, seed=0x5EED10F6, lq=2048, ld=2000):
    """2,048 x 2,000 G-mut(5%) pairs: 1,600 db rows of the query's mutated
    middle inside a random window."""
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


def batch_call(entry, q_seq, q_off, d_seq, d_off, pq, pd, mode, scoring_arg, want_cigar):
    """A closure that makes one call of the C entry point `entry`
    (saln_ends_free_align_batch and its _long and _replay kin) on host buffers
    and frees the handle it returns."""
    from sequencealigning_amd import _lib
    L, ctx = _lib.lib(), _lib.context(0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

    def run():
        h = C.c_void_p()
        _lib.check(getattr(L, entry)(
            ctx, vp(q_seq), vp(q_off), len(q_off) - 1, vp(d_seq), vp(d_off), len(d_off) - 1,
            vp(pq), vp(pd), len(pq), mode, scoring_arg, 0, int(want_cigar), C.byref(h)), entry)
        L.saln_ends_free_aln_free(h)
    return run


def model_check(got, cig, qs, ds, mode, scoring, cigar):
    """True when record k of `got` (and, cig given, its words) is the plain
    model's alignment of qs[k] with ds[k], for every k."""
    import ends_free_model as model
    ok = True
    for k in range(len(got)):
        m = model.align(qs[k], ds[k], mode, scoring, walk=cigar)
        ok &= tuple(int(v) for v in got[k]) == m.record()
        if cig is not None:
            ok &= cig.words(k).tolist() == model.cigar_words(m.cigar)
    return bool(ok)
