"""Host model of the fire verdicts (cg_expand_verdicts_device): the two literal
processes of the admission and the lock profile, fire by fire, as one byte per
fire of a rule-major CSR.

Plain numpy and Python integers, no call into the library.
  bit 0 (DROPPED)  admit = (dur_ms, parallels, unit): a unit's fires in (time,
                   rule index) order; a fire at t is admitted iff P == 0 or
                   fewer than P admitted fires a of the unit have
                   a * 1000 + dur_ms > t * 1000, else dropped.  The duration is
                   rounded up to whole seconds and clamped to t1 - t0 first, as
                   the engine does (inside the horizon that changes nothing).
  bit 1 (SKIPPED)  lock = (kind, avg_ms, unit, contends): the contending fires of
                   a unit of kind ALONE / INTERVAL in (time, rule index) order
                   with free_at = -infinity; t < free_at: skipped; ttl =
                   ttl_of(rule, t) == 0: skipped, state unchanged; else granted
                   and free_at = t + ttl (INTERVAL) or t + d + ttl (ALONE, d =
                   ceil(max(avg, 0) / 1000)).  ttl_of None: LockStuck.
The bits are independent.  test_verdict_model.py pins the model to hand-derived
cases; the host check and the GPU tests hold the engine to it.
"""
from collections import deque

import numpy as np

from admit_model import units_of
from lock_model import ALONE, COMMON, INTERVAL, LockStuck

DROPPED, SKIPPED = 1, 2


def _seconds(ms, horizon):
    return min(ms // 1000 + (1 if ms % 1000 else 0), horizon)


def _unit_fires(off, times, rows):
    """(times, rules) of the rows' fires in (time, rule) order, with their CSR indices."""
    if not rows:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    idx = np.concatenate([np.arange(off[r], off[r + 1], dtype=np.int64) for r in rows])
    rs = np.concatenate([np.full(int(off[r + 1] - off[r]), r, dtype=np.int64) for r in rows])
    ts = times[idx]
    order = np.lexsort((rs, ts))
    return ts[order], rs[order], idx[order]


def verdicts_from_lists(off, times, t0, t1, admit=None, lock=None, ttl_of=None):
    """uint8 [E]: the verdict byte of every fire of the CSR (off [K+1], times
    sorted per rule, all in (t0, t1])."""
    K = len(off) - 1
    off = np.asarray(off, dtype=np.int64)
    times = np.asarray(times, dtype=np.int64)
    E = int(off[K])
    assert times.shape[0] >= E and (E == 0 or (t0 < times[:E].min() and times[:E].max() <= t1))
    out = np.zeros(E, dtype=np.uint8)
    if admit is not None:
        dur_ms, parallels, unit = admit
        for u0, u1 in units_of(unit, K):
            ms, P = int(dur_ms[u0]), int(parallels[u0])
            assert all(int(dur_ms[r]) == ms and int(parallels[r]) == P for r in range(u0, u1)), "mixed unit"
            assert ms >= 0 and P >= 0
            if P == 0:
                continue
            d = _seconds(ms, t1 - t0)
            ts, rs, idx = _unit_fires(off, times, list(range(u0, u1)))
            running = deque()  # admitted starts that may still be running
            for t, e in zip(ts.tolist(), idx.tolist()):
                while running and running[0] + d <= t:
                    running.popleft()  # a fire at the second an instance ends is admitted
                if len(running) < P:
                    running.append(t)
                else:
                    out[e] |= DROPPED
    if lock is not None:
        kind, avg_ms, unit, contends = lock
        cont = np.ones(K, dtype=bool) if contends is None else np.asarray(contends).astype(bool)
        assert cont.shape == (K,)
        for u0, u1 in units_of(unit, K):
            kd, avg = int(kind[u0]), int(avg_ms[u0])
            assert kd in (COMMON, ALONE, INTERVAL)
            assert all(int(kind[r]) == kd and int(avg_ms[r]) == avg for r in range(u0, u1)), "mixed unit"
            if kd == COMMON:
                continue
            d = _seconds(max(avg, 0), t1 - t0)
            ts, rs, idx = _unit_fires(off, times, [r for r in range(u0, u1) if cont[r]])
            free_at = None  # None: -infinity
            for t, r, e in zip(ts.tolist(), rs.tolist(), idx.tolist()):
                if free_at is not None and t < free_at:
                    out[e] |= SKIPPED
                    continue
                ttl = ttl_of(r, t)
                if ttl is None:
                    raise LockStuck(r, t)
                if ttl == 0:
                    out[e] |= SKIPPED  # lock() returns nil: the key is untouched
                    continue
                free_at = t + ttl + (d if kd == ALONE else 0)
    return out


def select(off, times, verdict, mask, value):
    """(sel_off [K+1], sel_times): the rule-major CSR of the fires with
    (verdict & mask) == value."""
    K = len(off) - 1
    E = int(off[K])
    hit = (np.asarray(verdict[:E]) & mask) == value
    rule = np.repeat(np.arange(K, dtype=np.int64), np.diff(np.asarray(off, dtype=np.int64)))
    cnt = np.bincount(rule[hit], minlength=K).astype(np.int64)[:K]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), np.asarray(times[:E], dtype=np.int64)[hit]


def first_diff(off, got, exp):
    """'rule r fire i: got vs exp' of the first differing byte / time, or None."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return f"shape {got.shape} vs {exp.shape}"
    bad = np.nonzero(got != exp)[0]
    if bad.size == 0:
        return None
    e = int(bad[0])
    r = int(np.searchsorted(np.asarray(off), e, side="right") - 1)
    return f"rule {r} fire {e - int(off[r])}: {int(got[e])} vs {int(exp[e])}"
