"""The dispatcher's wake loop (Cron.run, node/cron/cron.go:210-275, restated by
the oracle's or_cron_*) as numpy array math, for tables too large to marshal
through oracle_lib.OracleCron entry by entry.

A slot holds Next, Prev (int64 unix seconds, O.ZERO_TIME for the zero time),
`live`, and a schedule that is one of
  * a whole-second delay (constantdelay.go:25-27: Next = now + d), kept as
    seconds in `delay` and advanced with array arithmetic, or
  * an oracle schedule (O.OrSched), kept as an index into `pool` and advanced
    with O.sched_next(pool[k], now, loc), one oracle call per distinct
    (schedule, now): a wake costs one call per distinct spec due.

tests/test_dispatch_model.py pins this file to O.OracleCron on the CPU; the GPU
tests then hold cg_dispatcher_* to it.  No GPU import here.

A schedule whose Next never returns (O.sched_next gives the oracle's
no-progress value) is not represented: advancing one raises.  A test that needs
such a slot swaps the slot's schedule for a never-firing one (Next = zero time)
before the wake that would hit it, which is the state the product documents.
"""
from collections import namedtuple

import numpy as np

import oracle_lib as O

Z = O.ZERO_TIME
NO_PROGRESS = -(1 << 63) + 1  # OR_NO_PROGRESS

# schedules for many slots at once: delay[j] > 0 (whole seconds) is a delay
# row, else spec[j] indexes the model's pool
Rows = namedtuple("Rows", "delay spec")


def _key(s):
    return (s.kind, s.spec.second, s.spec.minute, s.spec.hour, s.spec.dom, s.spec.month,
            s.spec.dow, s.delay_ns)


class DispatchModel:
    def __init__(self, loc, schedules=()):
        """loc: an oracle location (common.oracle_zone).  schedules: see rows()."""
        self.loc = loc
        self.pool = []
        self._pool_ix = {}
        self._cache = {}
        self.oracle_calls = 0
        r = self.rows(schedules)
        n = len(r.delay)
        self.delay = r.delay.copy()
        self.spec = r.spec.copy()
        self.next = np.full(n, Z, dtype=np.int64)
        self.prev = np.full(n, Z, dtype=np.int64)
        self.live = np.ones(n, dtype=bool)

    def __len__(self):
        return len(self.next)

    # ------------------------------------------------------------ schedules
    def intern(self, sched):
        """Pool index of an oracle schedule (equal schedules share one)."""
        k = _key(sched)
        ix = self._pool_ix.get(k)
        if ix is None:
            ix = self._pool_ix[k] = len(self.pool)
            self.pool.append(sched)
        return ix

    def rows(self, schedules):
        """Rows from Rows, or from a sequence of whole-second delays (int) and
        oracle schedules (O.OrSched) in any mix."""
        if isinstance(schedules, Rows):
            d = np.ascontiguousarray(schedules.delay, dtype=np.int64)
            s = np.ascontiguousarray(schedules.spec, dtype=np.int32)
            assert d.shape == s.shape and d.ndim == 1
            assert np.all((d > 0) | ((s >= 0) & (s < len(self.pool))))
            return Rows(d, s)
        d = np.zeros(len(schedules), dtype=np.int64)
        s = np.full(len(schedules), -1, dtype=np.int32)
        for j, x in enumerate(schedules):
            if isinstance(x, O.OrSched):
                s[j] = self.intern(x)
            else:
                assert int(x) > 0
                d[j] = int(x)
        return Rows(d, s)

    def _pool_next(self, k, now):
        t = self._cache.get((k, now))
        if t is None:
            self.oracle_calls += 1
            t = O.sched_next(self.pool[k], now, self.loc)
            if t == NO_PROGRESS:
                raise ValueError(f"pool schedule {k}: Next({now}) never returns")
            self._cache[(k, now)] = t
        return t

    def _next_of(self, slots, now):
        """Schedule.Next(now) of each slot in `slots`."""
        now = int(now)
        d = self.delay[slots]
        out = now + d
        sp = np.flatnonzero(d <= 0)
        if sp.size:
            k = self.spec[slots][sp]
            assert np.all(k >= 0), "an empty slot has no schedule"
            uniq, inv = np.unique(k, return_inverse=True)
            lut = np.array([self._pool_next(int(u), now) for u in uniq], dtype=np.int64)
            out[sp] = lut[inv]
        return out

    # ------------------------------------------------------------- the loop
    def start(self, now):
        """run() start (cron.go:212-215): Next = Next(now), Prev = zero."""
        self.next = self._next_of(np.arange(len(self)), now)
        self.prev[:] = Z

    def effective(self):
        """entries[0].Next after sort.Sort(byTime) (cron.go:220-230)."""
        m = self.next != Z
        return int(self.next[m].min()) if m.any() else Z

    def fire(self, now):
        """The timer fired at now >= effective (cron.go:234-244):
        (due slots ascending, new effective)."""
        e = self.effective()
        if e == Z:
            return np.zeros(0, dtype=np.int32), Z
        assert now >= e
        due = np.flatnonzero(self.next == e)
        self.prev[due] = e
        self.next[due] = self._next_of(due, now)
        return due.astype(np.int32), self.effective()

    def set(self, slots, schedules, now):
        """Add or replace (cron.go:246-252): Next = Next(now), Prev = zero,
        live.  Slots past the count extend the table; skipped slots are empty
        and not live."""
        slots = np.atleast_1d(np.asarray(slots, dtype=np.int64))
        r = self.rows(schedules)
        assert len(r.delay) == len(slots) and len(np.unique(slots)) == len(slots)
        assert slots.size and slots.min() >= 0
        top = int(slots.max()) + 1
        if top > len(self):
            g = top - len(self)
            self.next = np.concatenate([self.next, np.full(g, Z, dtype=np.int64)])
            self.prev = np.concatenate([self.prev, np.full(g, Z, dtype=np.int64)])
            self.live = np.concatenate([self.live, np.zeros(g, dtype=bool)])
            self.delay = np.concatenate([self.delay, np.zeros(g, dtype=np.int64)])
            self.spec = np.concatenate([self.spec, np.full(g, -1, dtype=np.int32)])
        self.delay[slots] = r.delay
        self.spec[slots] = r.spec
        self.next[slots] = self._next_of(slots, now)
        self.prev[slots] = Z
        self.live[slots] = True

    def remove(self, slots):
        """DelJob (cron.go:254-262): Next = Prev = zero, not live."""
        slots = np.atleast_1d(np.asarray(slots, dtype=np.int64))
        self.next[slots] = Z
        self.prev[slots] = Z
        self.live[slots] = False
        self.delay[slots] = 0
        self.spec[slots] = -1


def every(seconds):
    """The oracle schedule of `@every <seconds>s` (the general path for a delay)."""
    s, err = O.parse(f"@every {int(seconds)}s")
    assert err is None, err
    return s
