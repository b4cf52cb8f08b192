"""The running model (running_model.py) pinned: its fire-by-fire passes keep
exactly the fires admit_model / lock_model count as ADMITTED / GRANTED, its
count equals a brute-force triple loop on tiny cases, hand-derived rows, and
the identities the definition promises (running <= in flight; d == w, d == m*w
and d >= B*w against the start buckets; <= P per droppable unit and <= 1 per
ALONE unit at every edge).  CPU only."""
import numpy as np
import pytest

import admit_model as AM
import inflight_model as IM
import lock_model as LM
import oracle_lib as O
import running_model as RM
from common import oracle_parse_all, oracle_zone

T0 = 1767571217  # 2026-01-05 00:00:17 UTC
C, A, I = LM.COMMON, LM.ALONE, LM.INTERVAL
SPECS = ["* * * * * *", "*/7 * * * * *", "@every 11s", "0 * * * * *", "7,30,45 * * * * *", "*/2 * * * * *",
         "@every 90s", "0 0 0 30 Feb ?"]


def lists(specs, horizon, t0=T0):
    return O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + horizon, oracle_zone("UTC"))


def brute(fires, t0, w, B, dur_ms):
    """The definition as three loops, in ms, Python integers."""
    out = np.zeros((len(fires), B), dtype=np.int32)
    for r, fs in enumerate(fires):
        for b in range(B):
            e = t0 + (b + 1) * w
            out[r, b] = sum(1 for a in fs if a <= e and e * 1000 < a * 1000 + int(dur_ms[r]))
    return out


def test_every_second_ten_second_runs():
    """`* * * * * *` running 10 s with P = 1: one fire in ten starts, at every
    second edge exactly one command runs; P = 2 starts two in ten (+1, +2, then
    +11, +12): two run at every edge but the first (at +11 the run from +1 has
    ended and the one admitted at +11 has started), and in flight is 10 once
    it has ramped up."""
    off, times = lists(["* * * * * *"], 60)
    run, adm = RM.admit_running(off, times, T0, 1, 60, [10_000], [1])
    assert adm[0].tolist() == [int(b % 10 == 0) for b in range(60)] and run[0].tolist() == [1] * 60
    run, adm = RM.admit_running(off, times, T0, 1, 60, [10_000], [2])
    assert adm[0].tolist() == [int(b % 10 < 2) for b in range(60)]
    assert run[0].tolist() == [1] + [2] * 59
    infl = IM.inflight_from_lists(off, times, T0, 1, 60, [10])
    assert infl[0].tolist() == [min(b + 1, 10) for b in range(60)]
    # 10-s buckets, P = 1: the fire admitted at +10b+1 still runs at the edge +10(b+1), the one at the edge is dropped
    run, _ = RM.admit_running(off, times, T0, 10, 6, [10_000], [1])
    assert run[0].tolist() == [1] * 6
    # 10 001 ms: a fire in eleven starts; at the edge +10 the one from +1 still runs
    run, adm = RM.admit_running(off, times, T0, 1, 60, [10_001], [1])
    assert np.nonzero(adm[0])[0].tolist() == [0, 11, 22, 33, 44, 55] and run[0].tolist() == [1] * 60


@pytest.mark.parametrize("ms,cells", [(0, [0, 0, 0]), (999, [1, 1, 1]), (1000, [1, 1, 1]), (1001, [1, 1, 1])])
def test_around_one_second(ms, cells):
    """Edges are whole seconds and so are fires: a fire at the edge itself runs
    at it for any ms > 0; the one a second earlier has ended after 999 and
    1000 ms, and after 1001 ms it would still run -- but then P = 1 dropped
    the fire at the edge."""
    off, times = lists(["* * * * * *"], 3)
    run, _ = RM.admit_running(off, times, T0, 1, 3, [ms], [1])
    assert run[0].tolist() == cells
    run, _ = RM.admit_running(off, times, T0, 1, 3, [ms], [0])  # no limit: the in-flight profile
    assert run[0].tolist() == ([0, 0, 0] if ms == 0 else [1, 2, 2] if ms == 1001 else [1, 1, 1])


def test_alone_every_60s_runs_every_other_minute():
    """@every 60s ALONE, AvgTime 2500, ttl 58: granted at +60, +180, ...  With
    60-s buckets a granted run starts at an edge and so runs at it; with 1-s
    buckets it shows at three edges (2.5 s: +60, +61, +62)."""
    off, times = lists(["@every 60s"], 600)
    run, g = RM.lock_running(off, times, T0, 60, 10, [A], [2500], None, None, lambda r, t: 58)
    assert g[0].tolist() == [1, 0] * 5 and run[0].tolist() == [1, 0] * 5
    run, g = RM.lock_running(off, times, T0, 1, 600, [A], [2500], None, None, lambda r, t: 58)
    assert np.nonzero(run[0])[0].tolist() == [b for s in (60, 180, 300, 420, 540) for b in (s - 1, s, s + 1)]
    # INTERVAL with the same ttl: the lease ends at +58, every fire is granted, each runs 3 edges
    run, g = RM.lock_running(off, times, T0, 1, 600, [I], [2500], None, None, lambda r, t: 58)
    assert int(g.sum()) == 10 and int(run.sum()) == 9 * 3 + 1  # the last starts at the last edge
    # AvgTime <= 0: granted fires, nothing in flight
    run, g = RM.lock_running(off, times, T0, 60, 10, [I], [-1500], None, None, lambda r, t: 58)
    assert g.any() and not run.any()


def _random_case(seed):
    rng = np.random.default_rng(seed)
    sizes = [3, 1, 2, 2]
    K = sum(sizes)
    specs = [SPECS[i] for i in rng.integers(0, len(SPECS), K)]
    unit = np.repeat(np.arange(len(sizes)) * 2 + 1, sizes)
    return rng, sizes, specs, unit


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("w,B", [(1, 50), (7, 13), (60, 4)])
def test_against_brute_force_and_the_two_models(seed, w, B):
    """Tiny horizons, units of 3, 1, 2 and 2 rules: the kept fires binned by
    start equal admit_model's / lock_model's matrices, the vectorised count
    equals the triple loop, and the bounds hold."""
    rng, sizes, specs, unit = _random_case(seed)
    off, times = lists(specs, w * B)
    durs = [0, 999, 1001, w * 1000, 3 * w * 1000, (w * B + 9) * 1000, IM.INT64_MAX, 2500]
    dur = np.repeat([durs[i] for i in rng.integers(0, len(durs), len(sizes))], sizes).astype(np.int64)
    par = np.repeat(rng.integers(0, 4, len(sizes)), sizes).astype(np.int64)
    fires = RM.admitted_fires(off, times, dur, par, unit)
    run, adm = RM.admit_running(off, times, T0, w, B, dur, par, unit)
    assert np.array_equal(adm, AM.admit_from_lists(off, times, T0, w, B, dur, par, unit)[0])
    assert np.array_equal(run, brute(fires, T0, w, B, dur))
    infl = IM.inflight_from_lists(off, times, T0, w, B, IM.seconds(dur))
    assert (run <= infl).all()
    sums = RM.unit_sums(run, unit)
    for u, (a, _) in enumerate(AM.units_of(unit, len(specs))):
        if par[a] > 0:
            assert sums[u].max(initial=0) <= par[a], (u, sums[u].max())
        if AM.never_drops(int(par[a]), int(min(IM.seconds(dur)[a], w * B)), sizes[u]):
            assert np.array_equal(run[a:a + sizes[u]], infl[a:a + sizes[u]])
    # the lock flavour with a stub ttl
    kind = np.repeat(rng.integers(0, 3, len(sizes)), sizes).astype(np.int32)
    avg = np.where(dur > 10**15, dur, dur - 1500)  # some negative
    contends = rng.integers(0, 4, len(specs)) > 0

    def ttl_of(r, t):
        return (r + t) % 5 * 3  # 0 among them: skipped, the key untouched
    gf = RM.granted_fires(off, times, kind, avg, unit, contends, ttl_of)
    lrun, g = RM.lock_running(off, times, T0, w, B, kind, avg, unit, contends, ttl_of)
    assert np.array_equal(g, LM.lock_from_lists(off, times, T0, w, B, kind, avg, unit, contends, ttl_of)[0])
    assert np.array_equal(lrun, brute(gf, T0, w, B, np.maximum(avg, 0)))
    linfl = IM.inflight_from_lists(off, times, T0, w, B, IM.seconds(np.maximum(avg, 0)))
    assert (lrun <= linfl).all()
    for a, b in AM.units_of(unit, len(specs)):
        for r in range(a, b):
            if kind[a] == C or not contends[r]:
                assert np.array_equal(lrun[r], linfl[r])


@pytest.mark.parametrize("m", [1, 2, 5])
def test_whole_bucket_durations_are_sliding_sums_of_the_starts(m):
    """d == w gives the ADMITTED (GRANTED) rows, d == m*w the sliding sum of m
    of their buckets, d >= B*w the prefix sums."""
    w, B = 20, 30
    off, times = lists(SPECS, w * B)
    K = len(SPECS)
    unit = np.array([0, 0, 0, 1, 1, 2, 3, 4])
    par = np.array([1, 1, 1, 2, 2, 1, 0, 1], dtype=np.int64)
    for ms, mm in ((m * w * 1000, m), (w * B * 1000, B), (IM.INT64_MAX, B)):
        dur = np.full(K, ms, dtype=np.int64)
        run, adm = RM.admit_running(off, times, T0, w, B, dur, par, unit)
        assert np.array_equal(run, IM.sliding_sum(adm, mm))
        kind = np.array([A, A, A, I, I, C, A, I], dtype=np.int32)
        lrun, g = RM.lock_running(off, times, T0, w, B, kind, dur, unit, None, lambda r, t: 2 + (t % 3))
        assert np.array_equal(lrun, IM.sliding_sum(g, mm))
        sums = RM.unit_sums(lrun, unit)
        assert sums[0].max() <= 1 and sums[4].max() <= 1  # ALONE: free_at = g + d + ttl


def test_lock_stuck_is_raised():
    off, times = lists(["@every 60s"], 600)
    with pytest.raises(LM.LockStuck):
        RM.lock_running(off, times, T0, 60, 10, [A], [0], None, None, lambda r, t: None)
