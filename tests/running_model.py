"""Host model of the running profile (CG_PROFILE_RUNNING of cg_admit_*,
CG_PROFILE_LOCK_RUNNING of cg_lock_profile_*): commands in flight at each
bucket edge, counting only the fires that start.

Plain numpy and Python integers, no call into the library.  Two steps, both
literal.  A fire-by-fire pass in (time, rule) order keeps the fires that start
-- admit_model's process for the admission flavour, lock_model's for the lock
flavour, with the same arguments; test_running_model.py holds the kept fires,
binned by start bucket, to those two models' own matrices.  Then, with the
bucket edges e_b = t0 + (b+1)*w, cell [r, b] counts the kept fires a of rule r
with a <= e_b and e_b*1000 < a*1000 + dur_ms: started and not yet finished at
the edge, in ms, with no rounding and no clamp.
"""
from collections import deque

import numpy as np

from admit_model import units_of
from lock_model import ALONE, COMMON, INTERVAL, LockStuck


def _unit_fires(off, times, rows):
    """The fires of the given rules in (time, rule) order: (times, rules) lists."""
    if not rows:
        return [], []
    ts = np.concatenate([times[off[r]:off[r + 1]] for r in rows])
    rs = np.concatenate([np.full(int(off[r + 1] - off[r]), r, dtype=np.int64) for r in rows])
    order = np.lexsort((rs, ts))
    return ts[order].tolist(), rs[order].tolist()


def admitted_fires(off, times, dur_ms, parallels, unit=None):
    """Per rule the list of its fires Job.limit() admits (admit_model's
    process: fewer than P admitted fires a of the unit with a*1000 + dur_ms >
    t*1000)."""
    K = len(off) - 1
    times = np.asarray(times, dtype=np.int64)
    out = [[] for _ in range(K)]
    for u0, u1 in units_of(unit, K):
        ms, P = int(dur_ms[u0]), int(parallels[u0])
        assert all(int(dur_ms[r]) == ms and int(parallels[r]) == P for r in range(u0, u1)), "mixed unit"
        assert ms >= 0 and P >= 0
        busy = deque()
        for t, r in zip(*_unit_fires(off, times, list(range(u0, u1)))):
            while busy and busy[0] * 1000 + ms <= t * 1000:
                busy.popleft()
            if P == 0 or len(busy) < P:
                if P:
                    busy.append(t)
                out[r].append(t)
    return out


def granted_fires(off, times, kind, avg_ms, unit, contends, ttl_of):
    """Per rule the list of its fires that run under the job lock
    (lock_model's process); every fire of a COMMON unit's rule and of a
    non-contending rule."""
    K = len(off) - 1
    times = np.asarray(times, dtype=np.int64)
    cont = np.ones(K, dtype=bool) if contends is None else np.asarray(contends).astype(bool)
    out = [[] for _ in range(K)]
    for u0, u1 in units_of(unit, K):
        kd, avg = int(kind[u0]), int(avg_ms[u0])
        assert kd in (COMMON, ALONE, INTERVAL)
        assert all(int(kind[r]) == kd and int(avg_ms[r]) == avg for r in range(u0, u1)), "mixed unit"
        rows = [r for r in range(u0, u1) if kd != COMMON and cont[r]]
        for r in range(u0, u1):
            if r not in rows:
                out[r] = times[off[r]:off[r + 1]].tolist()
        free_ms = None  # the lease's end in ms; None: -infinity
        for t, r in zip(*_unit_fires(off, times, rows)):
            if free_ms is not None and t * 1000 < free_ms:
                continue
            ttl = ttl_of(r, t)
            if ttl is None:
                raise LockStuck(r, t)
            if ttl == 0:
                continue
            out[r].append(t)
            free_ms = t * 1000 + ttl * 1000 + (max(avg, 0) if kd == ALONE else 0)
    return out


def bin_starts(fires, t0, w, B):
    """int32 [K, B]: the kept fires by start bucket (the ADMITTED / GRANTED matrix)."""
    out = np.zeros((len(fires), B), dtype=np.int32)
    for r, fs in enumerate(fires):
        if fs:
            np.add.at(out[r], (np.asarray(fs, dtype=np.int64) - t0 - 1) // w, 1)
    return out


def running_from_fires(fires, t0, w, B, dur_ms):
    """int32 [K, B]: cell [r, b] = #{a in fires[r] : a <= e_b and e_b*1000 <
    a*1000 + dur_ms[r]}, e_b = t0 + (b+1)*w.  The second test is taken as
    (e_b - a)*1000 < dur_ms, which is the same and cannot overflow at
    dur_ms = INT64_MAX."""
    e = t0 + (np.arange(B, dtype=np.int64) + 1) * w
    out = np.zeros((len(fires), B), dtype=np.int32)
    for r, fs in enumerate(fires):
        ms = int(dur_ms[r])
        assert ms >= 0
        if not fs or ms == 0:
            continue
        a = np.asarray(fs, dtype=np.int64)
        for i in range(0, len(a), 2048):  # blocks of fires x all edges
            gap = e[None, :] - a[i:i + 2048, None]
            out[r] += ((gap >= 0) & (gap * 1000 < ms)).sum(axis=0, dtype=np.int32)
    return out


def admit_running(off, times, t0, w, B, dur_ms, parallels, unit=None):
    """(running int32 [K, B], admitted int32 [K, B]) of the admission flavour."""
    fires = admitted_fires(off, times, dur_ms, parallels, unit)
    return running_from_fires(fires, t0, w, B, dur_ms), bin_starts(fires, t0, w, B)


def lock_running(off, times, t0, w, B, kind, avg_ms, unit, contends, ttl_of):
    """(running int32 [K, B], granted int32 [K, B]) of the lock flavour: every
    command runs max(AvgTime, 0) ms, whatever its kind and its lease."""
    fires = granted_fires(off, times, kind, avg_ms, unit, contends, ttl_of)
    dur = np.maximum(np.asarray(avg_ms, dtype=np.int64), 0)
    return running_from_fires(fires, t0, w, B, dur), bin_starts(fires, t0, w, B)


def unit_sums(matrix, unit):
    """int64 [units, B]: the rows of each unit summed (the <= P and <= 1 bounds)."""
    return np.array([matrix[a:b].sum(axis=0, dtype=np.int64) for a, b in units_of(unit, matrix.shape[0])])
