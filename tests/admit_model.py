"""Host model of the admission profile (cg_admit_*): the literal process of
the definition, fire by fire.

Plain numpy and Python integers, no call into the library.  Rules with equal
`unit` (non-decreasing along the rules; None: every rule alone) share one
limit.  A unit's fires in (t0, t0 + B*w] are taken in order of (time, rule
index); with P = parallels and dur_ms of the unit, a fire at t is admitted iff
P == 0 or fewer than P already admitted fires a of the unit have
a * 1000 + dur_ms > t * 1000 (started and not yet finished), else dropped.
test_admit_model.py pins it to hand-derived cases; the host check of the shared
routine and the GPU tests hold the engine to the same process.
"""
from collections import deque

import numpy as np


def units_of(unit, K):
    """[(u0, u1), ...]: the maximal runs of equal unit (None: one per rule)."""
    if unit is None:
        return [(r, r + 1) for r in range(K)]
    unit = np.asarray(unit)
    assert unit.shape == (K,) and (K < 2 or (np.diff(unit) >= 0).all()), "unit must not decrease"
    cuts = [0] + [int(i) + 1 for i in np.nonzero(np.diff(unit))[0]] + [K]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def admit_from_lists(off, times, t0, w, B, dur_ms, parallels, unit=None):
    """(admitted, dropped): int32 [K, B] each, from a CSR of sorted fire lists
    (off [K+1], times in (t0, t0 + B*w])."""
    K = len(off) - 1
    times = np.asarray(times, dtype=np.int64)
    adm = np.zeros((K, B), dtype=np.int32)
    drop = np.zeros((K, B), dtype=np.int32)
    for u0, u1 in units_of(unit, K):
        ms, P = int(dur_ms[u0]), int(parallels[u0])
        assert all(int(dur_ms[r]) == ms and int(parallels[r]) == P for r in range(u0, u1)), "mixed unit"
        assert ms >= 0 and P >= 0
        ts = times[off[u0]:off[u1]]
        rs = np.repeat(np.arange(u0, u1), np.diff(off[u0:u1 + 1]))
        order = np.lexsort((rs, ts))  # time ascending, then rule ascending
        running = deque()  # admitted starts that may still be running
        for t, r in zip(ts[order].tolist(), rs[order].tolist()):
            while running and running[0] * 1000 + ms <= t * 1000:
                running.popleft()  # finished: a fire at the second an instance ends is admitted
            b = (t - t0 - 1) // w
            assert 0 <= b < B
            if P == 0 or len(running) < P:
                if P:
                    running.append(t)
                adm[r, b] += 1
            else:
                drop[r, b] += 1
    return adm, drop


def never_drops(P, d_sec, k):
    """The engine's shortcut: no limit, no run time, or a limit k rules firing
    at most once a second each cannot reach."""
    return P == 0 or d_sec == 0 or P >= k * d_sec
