"""Host model of the lock profile (cg_lock_profile_*): the literal process of
the definition, fire by fire.

Plain numpy and Python integers, no call into the library.  Rules with equal
`unit` (non-decreasing along the rules; None: every rule alone) are one job; a
unit of kind ALONE or INTERVAL is a lock unit.  The fires of its contending
rules in (t0, t0 + B*w] are taken in order of (time, rule index) with the state
free_at = -infinity:
  t < free_at          skipped
  ttl = ttl_of(r, t)   0: skipped, state unchanged; None: the reference's
                       lockTtl never returns (LockStuck)
  else                 granted; free_at = t + ttl (INTERVAL), or the lease ends
                       at t*1000 + max(avg_ms, 0) + ttl*1000 ms (ALONE)
Rows of COMMON units and of non-contending rules: granted is the start row,
skipped zero.  ttl_of(rule, t) is a callable: a stub in test_lock_model.py, the
oracle's lock_ttl at now = t in the GPU tests.
"""
import numpy as np

from admit_model import units_of

COMMON, ALONE, INTERVAL = 0, 1, 2


class LockStuck(Exception):
    """ttl_of returned None: Next never returns from a fire that finds the key gone."""

    def __init__(self, rule, t):
        super().__init__(f"rule {rule} at {t}")
        self.rule, self.t = rule, t


def lock_from_lists(off, times, t0, w, B, kind, avg_ms, unit, contends, ttl_of):
    """(granted, skipped): int32 [K, B] each, from a CSR of sorted fire lists
    (off [K+1], times in (t0, t0 + B*w])."""
    K = len(off) - 1
    times = np.asarray(times, dtype=np.int64)
    granted = np.zeros((K, B), dtype=np.int32)
    skipped = np.zeros((K, B), dtype=np.int32)
    cont = np.ones(K, dtype=bool) if contends is None else np.asarray(contends).astype(bool)
    assert cont.shape == (K,)

    def bins(r):
        row = np.zeros(B, dtype=np.int32)
        ts = times[off[r]:off[r + 1]]
        np.add.at(row, (ts - t0 - 1) // w, 1)
        return row
    for u0, u1 in units_of(unit, K):
        kd, avg = int(kind[u0]), int(avg_ms[u0])
        assert kd in (COMMON, ALONE, INTERVAL)
        assert all(int(kind[r]) == kd and int(avg_ms[r]) == avg for r in range(u0, u1)), "mixed unit"
        rows = [r for r in range(u0, u1) if kd != COMMON and cont[r]]
        for r in range(u0, u1):
            if r not in rows:
                granted[r] = bins(r)
        if not rows:
            continue
        ts = np.concatenate([times[off[r]:off[r + 1]] for r in rows])
        rs = np.concatenate([np.full(int(off[r + 1] - off[r]), r, dtype=np.int64) for r in rows])
        order = np.lexsort((rs, ts))  # time ascending, then rule ascending
        free_ms = None  # the lease's end in ms; None: -infinity
        for t, r in zip(ts[order].tolist(), rs[order].tolist()):
            b = (t - t0 - 1) // w
            assert 0 <= b < B
            if free_ms is not None and t * 1000 < free_ms:
                skipped[r, b] += 1
                continue
            ttl = ttl_of(r, t)
            if ttl is None:
                raise LockStuck(r, t)
            if ttl == 0:
                skipped[r, b] += 1
                continue
            granted[r, b] += 1
            free_ms = t * 1000 + ttl * 1000 + (max(avg, 0) if kd == ALONE else 0)
    return granted, skipped
