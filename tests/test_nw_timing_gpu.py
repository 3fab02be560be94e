"""GPU: timed NW executes (saln_nw_plan_set_timing / _kernel_time).  Under
nw.timing_mode = 0 a pipelined plan of packed fill variants has its kernels
stamp the device's wall clock into a slot of the plan's stamp pool
(nw_stamps.hpp, nw_common.hpp stamp_begin / stamp_end); every other plan, and
every plan under nw.timing_mode = 1 (the default), records hipEvents.  Timing
never changes an output word, the counts equal the executes, and the stamped
spans obey the orderings the streams impose (no tolerances: the fills are
serial on one stream, a walk follows its fill).
Only stamped plans serve "nw_fill_gap", which is how a test tells the paths
apart.  The HIP-free half is tests/test_nw_stamps.py."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("nw_fill", "nw_traceback", "nw_execute", "nw_fill_gap", "nw_handoff")


def _batch(lens_q, ld, seed):
    """Pairs k = (query k, db k): offsets and random bases."""
    from sequencealigning_amd import synth
    lq = np.asarray(lens_q, np.int64)
    qo = np.concatenate([[0], np.cumsum(lq)]).astype(np.uint64)
    do = np.concatenate([[0], np.cumsum(np.full(len(lq), ld, np.int64))]).astype(np.uint64)
    return synth.random_bases(seed, int(qo[-1])), qo, synth.random_bases(seed + 1, int(do[-1])), do


def _run(saln, batch, *, steps, async_=True, timing=True, mode=0, score_only=False):
    """`steps` executes of one plan created under nw.timing_mode = mode:
    (outputs per step, {name: (ms, launches)}, host wall seconds from the
    first execute to the final synchronize)."""
    import torch
    qs, qo, ds, do = batch
    n = len(qo) - 1
    dq, dd = torch.from_numpy(qs).cuda(), torch.from_numpy(ds).cuda()
    with saln.options(**{"nw.timing_mode": mode}):
        plan = saln.NwPlan(qo, do, pairs=np.stack([np.arange(n)] * 2, 1))
    plan.set_async(async_)
    plan.set_score_only(score_only)
    plan.set_timing(timing)
    torch.cuda.synchronize()
    outs = []
    t0 = time.perf_counter()
    for _ in range(steps):
        r = torch.full((n * 4,), -1, dtype=torch.int32, device="cuda")
        c = torch.zeros(max(1, plan.cigar_words), dtype=torch.int32, device="cuda")
        plan.execute(dq, dd, r, None if score_only else c)
        outs.append((r, c))
    plan.sync()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    plan.check()
    times = {nm: plan.kernel_time(nm) for nm in NAMES}
    plan.close()
    return outs, times, wall


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for (ra, ca), (rb, cb) in zip(a, b):
        assert torch.equal(ra, rb) and torch.equal(ca, cb)


def _check_stamped(times, wall, steps):
    for nm in ("nw_fill", "nw_traceback", "nw_execute", "nw_handoff"):
        assert times[nm][1] == steps, (nm, times[nm])
    assert times["nw_fill_gap"][1] == steps - 1, times["nw_fill_gap"]
    fill, walk, ex = (times[nm][0] for nm in ("nw_fill", "nw_traceback", "nw_execute"))
    assert fill > 0 and walk > 0
    assert ex >= fill and ex >= walk
    assert times["nw_fill_gap"][0] >= 0
    assert fill <= wall * 1e3, (fill, wall)  # the fills are serial on one stream


def _check_events(times, steps):
    for nm in ("nw_fill", "nw_traceback", "nw_execute"):
        assert times[nm][1] == steps and times[nm][0] > 0, (nm, times[nm])
    assert times["nw_fill_gap"] == (0.0, 0) and times["nw_handoff"] == (0.0, 0)


def test_stamped_equals_untimed_and_events(saln):
    """130 pairs of 40 x 40: three fill workgroups (the last one partial) and
    a two-wave walk grid beside the next fill, so two lanes walk a second
    pair.  Stamped = untimed = nw.timing_mode 1, word for word."""
    batch = _batch([40] * 130, 40, 0x5EED0071)
    steps = 5
    stamped, ts, wall = _run(saln, batch, steps=steps)
    untimed, tu, _ = _run(saln, batch, steps=steps, timing=False)
    events, te, _ = _run(saln, batch, steps=steps, mode=1)
    _same(stamped, untimed)
    _same(stamped, events)
    _same(stamped[:1] * steps, stamped)  # every execute gives the same words
    _check_stamped(ts, wall, steps)
    _check_events(te, steps)
    assert all(tu[nm] == (0.0, 0) for nm in NAMES)


def test_two_packed_variants_one_fill_span(saln):
    """Queries of 40 and of 155 columns: the 8 x 19 and the 16 x 10 groups
    both launch, and both fold into the execute's one fill span."""
    lens = [40 if k % 2 == 0 else 155 for k in range(130)]
    batch = _batch(lens, 40, 0x5EED0073)
    steps = 4
    stamped, ts, wall = _run(saln, batch, steps=steps)
    untimed, _, _ = _run(saln, batch, steps=steps, timing=False)
    _same(stamped, untimed)
    _check_stamped(ts, wall, steps)


def test_fallback_launch_and_empty_side(saln):
    """One pair holds an N (the table fill's fallback launch does real work,
    uncounted, between the fill span and the walk span) and one pair has an
    empty query (the generic walk stamps too)."""
    lens = [40] * 130
    lens[77] = 0
    qs, qo, ds, do = _batch(lens, 40, 0x5EED0075)
    qs[int(qo[5]) + 7] = ord("N")
    batch = (qs, qo, ds, do)
    steps = 4
    stamped, ts, wall = _run(saln, batch, steps=steps)
    untimed, _, _ = _run(saln, batch, steps=steps, timing=False)
    events, te, _ = _run(saln, batch, steps=steps, mode=1)
    _same(stamped, untimed)
    _same(stamped, events)
    _check_stamped(ts, wall, steps)
    _check_events(te, steps)


def test_pool_growth(saln):
    """70 executes in a row cross the pool's first 64 slots: every execute is
    counted once."""
    batch = _batch([40] * 130, 40, 0x5EED0077)
    stamped, ts, wall = _run(saln, batch, steps=70)
    _same(stamped[:1] * 70, stamped)
    _check_stamped(ts, wall, 70)


def test_per_execute_order_and_toggle(saln):
    """Each execute read back on its own: fill begin < fill end, walk begin >=
    fill begin, walk end >= fill end (as differences of the spans).  Then
    set_timing off and on: the totals start again."""
    import torch
    qs, qo, ds, do = _batch([40] * 130, 40, 0x5EED0079)
    n = 130
    dq, dd = torch.from_numpy(qs).cuda(), torch.from_numpy(ds).cuda()
    with saln.options(**{"nw.timing_mode": 0}):
        plan = saln.NwPlan(qo, do, pairs=np.stack([np.arange(n)] * 2, 1))
    plan.set_async(True)
    plan.set_timing(True)
    r = [torch.zeros(n * 4, dtype=torch.int32, device="cuda") for _ in range(2)]
    c = [torch.zeros(max(1, plan.cigar_words), dtype=torch.int32, device="cuda") for _ in range(2)]
    prev = {nm: 0.0 for nm in NAMES}
    for k in range(4):
        plan.execute(dq, dd, r[k % 2], c[k % 2])
        cur = {nm: plan.kernel_time(nm) for nm in NAMES}  # waits for the walk
        assert all(cur[nm][1] == k + 1 for nm in NAMES if nm != "nw_fill_gap")
        assert cur["nw_fill_gap"][1] == 0  # no neighbour within one read
        fill, walk, ex, hand = (cur[nm][0] - prev[nm] for nm in
                                ("nw_fill", "nw_traceback", "nw_execute", "nw_handoff"))
        assert fill > 0                 # fill begin < fill end
        assert fill + hand >= -1e-9     # walk begin >= fill begin
        assert hand + walk >= -1e-9     # walk end >= fill end
        assert abs(ex - (fill + hand + walk)) < 1e-6
        prev = {nm: cur[nm][0] for nm in NAMES}
    plan.set_timing(False)
    for k in range(2):
        plan.execute(dq, dd, r[k % 2], c[k % 2])
    plan.set_timing(True)
    assert all(plan.kernel_time(nm) == (0.0, 0) for nm in NAMES)
    for k in range(2):
        plan.execute(dq, dd, r[k % 2], c[k % 2])
    plan.sync()
    torch.cuda.synchronize()
    plan.check()
    assert plan.kernel_time("nw_fill")[1] == 2 and plan.kernel_time("nw_fill_gap")[1] == 1
    plan.close()


def test_sequential_and_score_only_keep_events(saln):
    """A sequential plan and a score-only plan that ask for stamps
    (nw.timing_mode = 0) still report through hipEvents: the
    three names, no stamped-only one; outputs as untimed."""
    batch = _batch([40] * 130, 40, 0x5EED007B)
    steps = 3
    seq, tq, _ = _run(saln, batch, steps=steps, async_=False)
    seq_u, _, _ = _run(saln, batch, steps=steps, async_=False, timing=False)
    _same(seq, seq_u)
    _check_events(tq, steps)
    so, to, _ = _run(saln, batch, steps=steps, score_only=True)
    so_u, _, _ = _run(saln, batch, steps=steps, score_only=True, timing=False)
    _same(so, so_u)
    _check_events(to, steps)
