"""The GPU-resident dispatcher (cg_dispatcher_*) against the oracle's Cron.run
wake loop (or_cron_*), wake by wake: the effective time, the set of entries
fired and every entry's Next/Prev, bit-exact, with adds and removes while
running and late wakes that skip missed fires.  Then the Cron mirror
(cronsun_amd.dispatch) through node/cron/cron_test.go's wall-clock cases.
Last, the same calls against the numpy model of the wake loop
(tests/dispatch_model.py) at the table sizes the oracle cannot marshal: bitmap
word and tile edges, 2.1M entries, growth with gaps, the zone table rebuild,
stuck entries, argument errors, and the batch kernels past their grid cap."""
import threading
import time
import zlib

import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, product_zone, random_spec

pytestmark = pytest.mark.gpu

Z = O.ZERO_TIME


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def _check_snapshot(d, oc):
    nx, pv, live = d.snapshot()
    snap = oc.snapshot()
    for i in range(len(nx)):
        if i in snap:
            assert live[i] and (int(nx[i]), int(pv[i])) == snap[i], (i, int(nx[i]), int(pv[i]), snap[i])
        else:
            assert not live[i]


# zones without skipped local days (where the reference Next never returns)
@pytest.mark.parametrize("zone,t0", [
    ("UTC", 1767225600),
    ("America/New_York", 1772953200 - 5400),    # 90 min before 2026-03-08 02:00 EST
    ("Australia/Lord_Howe", 1775314800 - 3600),  # before the 30-minute fall-back
    ("Europe/London", 1792890000 - 3600),
    ("Asia/Kathmandu", 1767225600),
])
def test_dispatcher_vs_oracle(eng, zone, t0):
    from cronsun_amd import cron
    rng = np.random.default_rng(zlib.crc32(b"dispatch" + zone.encode()))
    n = 1500
    specs = [random_spec(rng) for _ in range(n)]
    scheds = [cron.Parse(s) for s in specs]
    osch = oracle_parse_all(specs)  # the oracle's own parser
    oc = O.OracleCron(osch, oracle_zone(zone))
    z = product_zone(zone)
    oc.start(t0)
    d = eng.dispatcher(scheds, z, t0)
    _check_snapshot(d, oc)
    next_slot = n
    for w in range(120):
        e = oc.effective()
        assert d.effective == e, w
        if e == Z:
            break
        late = int(rng.choice([0, 0, 0, 1, 2, 59, 700, 4000]))
        now = e + late
        due, e2 = d.fire(now)
        assert [int(x) for x in due] == oc.fire(e, now), (w, e, now)
        assert e2 == oc.effective()
        if w % 15 == 7:  # add / replace / remove while running
            k = int(rng.integers(1, 6))
            slots = [int(x) for x in rng.choice(next_slot, k, replace=False)]
            if rng.random() < 0.5:
                slots.append(next_slot)
                next_slot += 1
            new_specs = [random_spec(rng) for _ in slots]
            new = [cron.Parse(x) for x in new_specs]
            d.set(slots, new, now)
            for s, osc in zip(slots, oracle_parse_all(new_specs)):
                oc.set(s, osc, now)
            rm = [int(x) for x in rng.choice(n, 3, replace=False) if int(x) not in slots]
            d.remove(rm)
            for s in rm:
                oc.remove(s)
        if w % 40 == 39:
            _check_snapshot(d, oc)
    _check_snapshot(d, oc)
    d.free()


def test_dispatcher_many_equal_due(eng):
    """A wake that fires most of a large table at once: the due list is the
    ascending slot list and the tile compaction covers every tile."""
    from cronsun_amd import cron
    n = 3 * 4096 + 123
    scheds = [cron.Every(60 * 10**9) if i % 7 else cron.Parse("0 0 * * * *") for i in range(n)]
    t0 = 1767225600
    d = eng.dispatcher(scheds, None, t0)
    assert d.effective == t0 + 60
    due, e2 = d.fire(t0 + 60)
    assert np.array_equal(due, np.array([i for i in range(n) if i % 7], dtype=np.int32))
    assert e2 == t0 + 120
    nx, pv, _ = d.snapshot()
    assert int(nx[1]) == t0 + 120 and int(pv[1]) == t0 + 60 and int(pv[0]) == Z
    d.free()


def test_dispatcher_empty_and_never(eng):
    from cronsun_amd import cron
    d = eng.dispatcher([cron.Parse("0 0 0 30 Feb ?")], None, 1767225600)
    assert d.effective == Z
    assert d.fire(1767225600 + 10)[0].size == 0
    d.set([5], [cron.Parse("@every 5s")], 1767225600)
    assert len(d) == 6 and d.effective == 1767225605
    nx, pv, live = d.snapshot()
    assert list(live) == [True, False, False, False, False, True]
    d.remove([5])
    assert d.effective == Z
    d.free()


# ------------------------------------------------ cron_test.go, wall clock
ONE_SECOND = 1.25  # cron_test.go:15 uses 1.01 s; a little slack for Python threads


class WG:
    """sync.WaitGroup"""

    def __init__(self, n):
        self.n = n
        self.cv = threading.Condition()

    def Done(self):
        with self.cv:
            self.n -= 1
            self.cv.notify_all()

    def wait(self, timeout):
        with self.cv:
            return self.cv.wait_for(lambda: self.n <= 0, timeout)


class NamedJob:
    """cron_test.go:280-291 testJob"""

    def __init__(self, wg, name):
        self.wg, self.name = wg, name

    def GetID(self):
        return self.name

    def Run(self):
        self.wg.Done()


def _boom():
    raise RuntimeError("YOLO")


def test_func_panic_recovery(eng):
    from cronsun_amd.dispatch import Cron
    c = Cron(engine=eng)
    c.Start()
    c.AddFunc("* * * * * ?", _boom)
    time.sleep(ONE_SECOND)
    c.Stop()


def test_no_entries_and_stop_without_start(eng):
    from cronsun_amd.dispatch import Cron
    Cron(engine=eng).Stop()
    c = Cron(engine=eng)
    c.Start()
    t = time.time()
    c.Stop()
    assert time.time() - t < ONE_SECOND


def test_stop_causes_jobs_to_not_run(eng):
    from cronsun_amd.dispatch import Cron
    wg = WG(1)
    c = Cron(engine=eng)
    c.Start()
    c.Stop()
    c.AddFunc("* * * * * ?", wg.Done)
    assert not wg.wait(ONE_SECOND)


def test_add_before_and_while_running(eng):
    from cronsun_amd.dispatch import Cron
    wg = WG(1)
    c = Cron(engine=eng)
    c.AddFunc("* * * * * ?", wg.Done)
    c.Start()
    assert wg.wait(ONE_SECOND)
    c.Stop()
    wg = WG(1)
    c = Cron(engine=eng)
    c.Start()
    c.AddFunc("* * * * * ?", wg.Done)
    assert wg.wait(ONE_SECOND)
    c.Stop()


def test_add_while_running_with_delay(eng):
    from cronsun_amd.dispatch import Cron
    c = Cron(engine=eng)
    c.Start()
    time.sleep(2)  # cron_test.go:123 sleeps 5 s
    calls = []
    c.AddFunc("* * * * * *", lambda: calls.append(1))
    time.sleep(1.01)
    c.Stop()
    assert len(calls) == 1


def test_snapshot_entries(eng):
    from cronsun_amd.dispatch import Cron
    wg = WG(1)
    c = Cron(engine=eng)
    c.AddFunc("@every 2s", wg.Done)
    c.Start()
    time.sleep(1.01)
    c.Entries()
    assert wg.wait(ONE_SECOND)
    c.Stop()


def test_multiple_entries_and_schedules(eng):
    from cronsun_amd import cron
    from cronsun_amd.dispatch import Cron, FuncJob
    wg = WG(4)
    c = Cron(engine=eng)
    c.AddFunc("0 0 0 1 1 ?", lambda: None)
    c.AddFunc("* * * * * ?", wg.Done)
    c.AddFunc("0 0 0 31 12 ?", lambda: None)
    f2 = lambda: wg.Done()  # noqa: E731
    c.AddFunc("* * * * * ?", f2)
    c.Schedule(cron.Every(60 * 10**9), FuncJob(lambda: None))
    f3 = lambda: wg.Done()  # noqa: E731
    c.Schedule(cron.Every(10**9), FuncJob(f3))
    c.Start()
    assert wg.wait(2 * ONE_SECOND)
    c.Stop()


def test_non_local_timezone(eng):
    from cronsun_amd import cron
    from cronsun_amd.dispatch import Cron
    loc = cron.FixedZone("Atlantic/Cape_Verde", -3600)  # cron_test.go:247-271
    wg = WG(2)
    lt = time.gmtime(int(time.time()) - 3600)
    if lt.tm_sec >= 57:  # keep both seconds inside this minute
        time.sleep(4)
        lt = time.gmtime(int(time.time()) - 3600)
    spec = f"{lt.tm_sec + 1},{lt.tm_sec + 2} {lt.tm_min} {lt.tm_hour} {lt.tm_mday} {lt.tm_mon} ?"
    c = Cron(loc, engine=eng)
    c.AddFunc(spec, wg.Done)
    c.Start()
    assert wg.wait(2 * ONE_SECOND), spec
    c.Stop()


def test_job_order(eng):
    from cronsun_amd import cron
    from cronsun_amd.dispatch import Cron
    wg = WG(1)
    c = Cron(engine=eng)
    c.AddJob("0 0 0 30 Feb ?", NamedJob(wg, "job0"))
    c.AddJob("0 0 0 1 1 ?", NamedJob(wg, "job1"))
    c.AddJob("* * * * * ?", NamedJob(wg, "job2"))
    c.AddJob("1 0 0 1 1 ?", NamedJob(wg, "job3"))
    c.Schedule(cron.Every(5 * 10**9 + 5), NamedJob(wg, "job4"))
    c.Schedule(cron.Every(5 * 60 * 10**9), NamedJob(wg, "job5"))
    c.Start()
    assert wg.wait(ONE_SECOND)
    assert [e.Job.name for e in c.Entries()] == ["job2", "job4", "job5", "job1", "job3", "job0"]
    c.Stop()


# ------------------------------------- the kernels against the host model --
# tests/dispatch_model.py (pinned to the oracle by tests/test_dispatch_model.py)
# at the sizes where the wake kernels take another path: see DESIGN.md §6.
import calendar  # noqa: E402
import ctypes as C  # noqa: E402

from dispatch_model import DispatchModel, Rows  # noqa: E402

T0 = 1767225600  # 2026-01-01 00:00:00 UTC
NO_PROGRESS = -(1 << 63) + 1
SCHED = np.dtype([("kind", "<i4"), ("reserved", "<i4"), ("second", "<u8"), ("minute", "<u8"),
                  ("hour", "<u8"), ("dom", "<u8"), ("month", "<u8"), ("dow", "<u8"),
                  ("delay_ns", "<i8")])  # cg_schedule


class Table:
    """A DispatchModel and the product's form of its rows: per pool schedule
    the six masks and delay of cron.Parse, gathered into SoA columns (upload)
    or a cg_schedule array (set) with array indexing, never per-row objects."""

    def __init__(self, zone):
        self.zone = zone
        self.m = DispatchModel(oracle_zone(zone))
        self.cols = np.zeros((0, 7), dtype=np.uint64)  # per pool index

    def spec(self, s):
        """Pool index of spec string s (the oracle's parser for the model,
        the product's for the device)."""
        from cronsun_amd import cron
        osc, err = O.parse(s)
        assert err is None, (s, err)
        k = self.m.intern(osc)
        if k == len(self.cols):
            p = cron.Parse(s)
            row = ([0] * 6 + [p.Delay] if isinstance(p, cron.ConstantDelaySchedule)
                   else [p.Second, p.Minute, p.Hour, p.Dom, p.Month, p.Dow, 0])
            self.cols = np.vstack([self.cols, np.array(row, dtype=np.uint64)])
        return k

    def rows(self, delay, spec):
        return Rows(np.asarray(delay, dtype=np.int64), np.asarray(spec, dtype=np.int32))

    def soa(self, r):
        """The seven upload_soa columns of rows r."""
        k = np.maximum(r.spec, 0)
        pool = self.cols[k] if len(self.cols) else np.zeros((len(k), 7), dtype=np.uint64)
        is_d = r.delay > 0
        masks = [np.where(is_d, np.uint64(0), pool[:, f]) for f in range(6)]
        return masks + [np.where(is_d, r.delay * 10**9, pool[:, 6].astype(np.int64))]

    def c_schedules(self, r):
        cols = self.soa(r)
        a = np.zeros(len(r.delay), dtype=SCHED)
        for f, name in enumerate(SCHED.names[2:]):
            a[name] = cols[f]
        a["kind"] = a["delay_ns"] > 0
        assert SCHED.itemsize == C.sizeof(_lib().cg_schedule)
        return (_lib().cg_schedule * len(a)).from_buffer(a)

    def start(self, eng, r, now):
        self.m = m = self._with_rows(r)
        m.start(now)
        self.d = eng.dispatcher(eng.upload_soa(*self.soa(r)), product_zone(self.zone), now)
        return self.d, m

    def _with_rows(self, r):
        m = self.m
        m.delay, m.spec = r.delay.copy(), r.spec.copy()
        n = len(r.delay)
        m.next = np.full(n, Z, dtype=np.int64)
        m.prev = np.full(n, Z, dtype=np.int64)
        m.live = np.ones(n, dtype=bool)
        return m

    def set(self, slots, r, now):
        self.m.set(slots, r, now)
        self.d.set(slots, self.c_schedules(r), now)

    def remove(self, slots):
        self.m.remove(slots)
        self.d.remove(slots)

    def wake(self, now, snapshot=True):
        """One wake of both at `now`: the due list and both effective times
        equal (and the whole snapshot); -> the due list."""
        assert self.d.effective == self.m.effective()
        due, e2 = self.d.fire(now)
        mdue, me2 = self.m.fire(now)
        _same_array(due, mdue, "due")
        assert e2 == me2 == self.d.effective
        if snapshot:
            self.same()
        return due

    def same(self, skip=()):
        nx, pv, live = self.d.snapshot()
        m = self.m
        assert len(nx) == len(m)
        if len(skip):
            keep = np.ones(len(m), dtype=bool)
            keep[list(skip)] = False
            nx, pv, mn, mp = nx[keep], pv[keep], m.next[keep], m.prev[keep]
        else:
            mn, mp = m.next, m.prev
        _same_array(nx, mn, "next")
        _same_array(pv, mp, "prev")
        _same_array(live, m.live, "live")
        assert self.d.effective == m.effective()


def _lib():
    from cronsun_amd import _lib as L
    return L


def _same_array(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} differ, first at {i}: {got[i]} != {exp[i]}")


# (a) word and tile edges of the due bitmap: one entry, whole words, whole
# tiles and one past each
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193])
def test_model_small_table_sweep(eng, n):
    t = Table("UTC")
    k10 = t.spec("0 */10 * * * *")
    i = np.arange(n)
    d, m = t.start(eng, t.rows(np.where(i % 3 == 2, 0, 600), np.where(i % 3 == 2, k10, -1)), T0)
    t.same()
    assert m.effective() == T0 + 600
    assert len(t.wake(T0 + 600)) == n  # every entry due
    t.set([n - 1], t.rows([7], [-1]), T0 + 600)
    assert t.wake(T0 + 607).tolist() == [n - 1]  # the last entry alone
    if n > 1:
        t.set([n - 1, 0], t.rows([600, 7], [-1, -1]), T0 + 607)
    assert t.wake(T0 + 614).tolist() == [0]  # the first entry alone
    d.free()


# (b) 514 scan tiles: past two passes of k_dispatch_compact's 256-wide loops,
# past the 4096 x 256 grid of advance / place / clear and past k_dispatch_min's
# 1024 x 2048
N_BIG = 513 * 4096 + 77
EDGES = [0, 63, 64, 4095, 4096, 256 * 4096 - 1, 256 * 4096, 257 * 4096 - 1, 512 * 4096 - 1,
         512 * 4096, 513 * 4096, 513 * 4096 + 63, 513 * 4096 + 64, N_BIG - 1]


def test_model_large_table(eng):
    rng = np.random.default_rng(20260101)
    t = Table("UTC")
    pool = []
    while len(pool) < 300:
        s = random_spec(rng)
        if O.parse(s)[1] is None:
            pool.append(t.spec(s))
    pool = np.array(pool, dtype=np.int32)
    n = N_BIG
    i = np.arange(n)
    delay = np.where(i % 5 == 4, 900, 600).astype(np.int64)
    spec = np.full(n, -1, dtype=np.int32)
    at = np.unique(np.concatenate([EDGES, rng.choice(n, 3000 - len(EDGES), replace=False)]))
    delay[at] = 0
    spec[at] = pool[rng.integers(0, len(pool), len(at))]
    # 1. creation
    d, m = t.start(eng, t.rows(delay, spec), T0)
    t.same()
    # 2. the edge slots fire every 7 s
    k7 = t.spec("@every 7s")
    t.set(EDGES, t.rows([0] * len(EDGES), [k7] * len(EDGES)), T0)
    # 3. sparse wakes on time: nearly every tile empty
    for _ in range(2):
        assert len(t.wake(m.effective(), snapshot=False)) < 3000
    # late from here on: every pending time below T0 + 600 takes one sparse
    # wake, the edge slots' T0 + 7 among them
    now = T0 + 600 + 59
    wakes = 0
    seen = np.zeros(n, dtype=bool)
    while m.effective() < T0 + 600:
        seen[t.wake(now, snapshot=False)] = True
        wakes += 1
        assert wakes < 600
    assert seen[EDGES].all()
    t.same()
    # 4. the wake of every 600 s row: a due list and an advance past the grid cap
    assert m.effective() == T0 + 600
    due = t.wake(now)
    assert len(due) > 1_600_000 and due[-1] > 513 * 4096
    # 5. the minimum alone in the last tile, then gone
    t.set([n - 3], t.rows([1], [-1]), T0 + 600)
    assert d.effective == m.effective() == T0 + 601
    t.remove([n - 3])
    assert d.effective == m.effective() > T0 + 601
    # 6. a set past the place kernel's grid cap, in no slot order
    k = 1 << 20 | 333
    slots = rng.permutation(n)[:k]
    j = np.arange(k)
    sd = np.where(j % 4 == 0, 300, 1200).astype(np.int64)
    ss = np.full(k, -1, dtype=np.int32)
    sd[j % 100 == 99] = 0
    ss[j % 100 == 99] = pool[rng.integers(0, len(pool), int((j % 100 == 99).sum()))]
    t.set(slots, t.rows(sd, ss), now)
    assert d.effective == m.effective()
    # 7. a last wake and every entry
    t.wake(m.effective())
    d.free()


# (c) growth by set: into the last slot of the capacity, one past it, and far
# past it with skipped slots
def test_model_growth_with_gaps(eng):
    t = Table("America/New_York")
    k = [t.spec(s) for s in ("*/5 * * * * *", "0 * * * * *", "@every 3s")]
    i = np.arange(1000)
    d, m = t.start(eng, t.rows(np.where(i % 4 == 0, 0, 60), np.where(i % 4 == 0, k[0], -1)), T0)
    t.same()
    now = T0
    for slots, r in [([1023], t.rows([2], [-1])),
                     ([1024], t.rows([0], [k[2]])),
                     ([9000, 40000], t.rows([4, 0], [-1, k[1]]))]:
        t.set(slots, r, now)
        assert len(d) == len(m) == max(slots) + 1
        t.same()
        for _ in range(3):
            now = m.effective()
            due = t.wake(now)
            assert m.live[due].all()
    assert int(m.live.sum()) == 1004 and not m.live[1000] and not m.live[39999]
    while m.effective() < T0 + 60:
        t.wake(m.effective(), snapshot=False)
    assert len(t.wake(T0 + 60)) >= 750  # the 60 s rows: the grown table's copy kept them
    d.free()


# (d) the zone table rebuilt forwards and backwards (cg_dispatcher::ensure_table)
def _utc(y, mo, dd, h=0):
    return calendar.timegm((y, mo, dd, h, 0, 0))


def test_zone_table_rebuild_vs_oracle(eng):
    from cronsun_amd import cron
    specs = ["0 30 2 * * *", "0 0 0 29 Feb *", "0 0 0 1 1 *", "0 30 1 1 11 *", "@every 8760h",
             "@every 36h"]
    zone = "America/New_York"
    oc = O.OracleCron(oracle_parse_all(specs), oracle_zone(zone))
    oc.start(T0)
    d = eng.dispatcher([cron.Parse(s) for s in specs], product_zone(zone), T0)
    day = 86400

    def wake(land=None):
        e = oc.effective()
        assert d.effective == e and e != Z
        now = e if land is None else land
        due, e2 = d.fire(now)
        assert [int(x) for x in due] == oc.fire(e, now), (e, now)
        assert e2 == oc.effective()
        _check_snapshot(d, oc)

    for _ in range(20):
        wake()
    wake(T0 + 3590 * day)  # the table built at T0 still serves this one
    wake(T0 + 3600 * day)  # and is rebuilt for this one
    # both 2036 transitions, then 2043-03-08: past the end (T0 + 16 * 366 d,
    # January 2042) of the table built at T0, which a table that was never
    # rebuilt would extend with its last offset
    for tr in (_utc(2036, 3, 9, 7), _utc(2036, 11, 2, 6), _utc(2043, 3, 8, 7)):
        wake(tr - 3 * day)
        while oc.effective() < tr - 3 * day:  # entries the late wake left behind
            wake(tr - 3 * day)
        for _ in range(12):
            wake()
        assert oc.effective() > tr
    # rebuilt backwards: 100 days before T0, then 300 days before it, where
    # the offset (EST, the day before 2025-03-09) differs from the first one
    # of every table built so far (EDT)
    for back in (T0 - 100 * day, T0 - 300 * day):
        d.set([3], [cron.Parse(specs[0])], back)
        oc.set(3, oracle_parse_all(specs[:1])[0], back)
        _check_snapshot(d, oc)
        assert oc.effective() < T0
        for _ in range(3):
            wake()
    wake(_utc(2044, 1, 1))  # and forwards again
    wake()
    d.free()


def test_next_batch_five_year_limit_past_2040(eng):
    """0 0 0 29 Feb * around 2100, which is no leap year: 2104-02-29 is
    within the reference's five-year search from some instants only."""
    from cronsun_amd import cron
    s = "0 0 0 29 Feb *"
    t = np.array([_utc(2096, 3, 1), _utc(2097, 1, 1), _utc(2099, 12, 31), _utc(2100, 2, 28)],
                 dtype=np.int64)
    got = eng.next_batch([cron.Parse(s)] * 4, None, t)
    osc = oracle_parse_all([s])[0]
    exp = [O.sched_next(osc, int(x), oracle_zone("UTC")) for x in t]
    assert [int(x) for x in got] == exp
    assert Z in exp and _utc(2104, 2, 29) in exp  # both sides of the limit


# (e) entries whose Next never returns: Pacific/Apia across the skipped
# 2011-12-30, the schedules and t0 of test_gpu_profile's
# test_apia_skipped_day_is_refused, where Engine.expand names rule 1
APIA = ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]
APIA_T0 = 1325030400
NEVER = "0 0 0 30 Feb ?"


def _apia_table(extra):
    t = Table("Pacific/Apia")
    k = [t.spec(s) for s in APIA + extra]
    return t, k, t.spec(NEVER)


def _rc_msg(rc):
    L = _lib()
    return rc, L.last_error()


def test_stuck_entry_at_new(eng):
    """cg_dispatcher_new names the lowest stuck slot and hands back a table
    whose other entries are placed; Engine.dispatcher frees it and raises."""
    L = _lib()
    t, k, never = _apia_table(["@every 90s"])
    r = t.rows([0] * 5, [k[0], k[1], k[2], k[1], k[3]])
    sp = eng.upload_soa(*t.soa(r))
    z = product_zone("Pacific/Apia")
    h = C.c_void_p()
    rc, msg = _rc_msg(L.lib().cg_dispatcher_new(eng._h, sp._h, z.handle, APIA_T0, C.byref(h)))
    assert rc == L.CG_ERANGE and "entry 1:" in msg and h
    from cronsun_amd.engine import Dispatcher
    t.d = Dispatcher(eng, h)
    m = t._with_rows(t.rows([0] * 5, [k[0], never, k[2], never, k[3]]))
    m.start(APIA_T0)
    t.same(skip=[1, 3])
    nx, pv, _ = t.d.snapshot()
    assert nx[[1, 3]].tolist() == [NO_PROGRESS] * 2 and pv[[1, 3]].tolist() == [Z] * 2
    t.wake(m.effective(), snapshot=False)
    t.same(skip=[1, 3])
    t.d.free()
    with pytest.raises(L.CgError) as e:
        eng.dispatcher(sp, z, APIA_T0)
    assert e.value.code == L.CG_ERANGE and "entry 1:" in e.value.msg


def test_stuck_entry_at_new_is_freed(eng):
    """Engine.dispatcher on a failed cg_dispatcher_new leaves no table in HBM:
    three failed 1M-entry tables (52 MB each) move free memory by less than
    one of them."""
    L = _lib()
    hip = C.CDLL(None)
    free, total = C.c_size_t(), C.c_size_t()

    def free_bytes():
        eng.sync()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    t, k, never = _apia_table([])
    n = 1 << 20
    spec = np.full(n, -1, dtype=np.int32)
    spec[n - 1] = k[1]
    sp = eng.upload_soa(*t.soa(t.rows(np.where(spec < 0, 60, 0), spec)))
    z = product_zone("Pacific/Apia")
    before = free_bytes()
    for _ in range(3):
        with pytest.raises(L.CgError) as e:
            eng.dispatcher(sp, z, APIA_T0)
        assert e.value.code == L.CG_ERANGE and f"entry {n - 1}:" in e.value.msg
    assert before - free_bytes() < 32 << 20


def test_stuck_entry_at_set_and_fire(eng):
    L = _lib()
    t, k, never = _apia_table(["0 0 9 * * *", "@every 6h"])
    # rule 1's Next returns up to 78 h before APIA_T0 (09:00 of the Saturday
    # before, 77 h before it) and is stuck from that fire on
    t0 = APIA_T0 - 100 * 3600
    stuck_at = APIA_T0 - 277200
    d, m = t.start(eng, t.rows([0] * 6, [k[0], k[1], k[2], k[3], k[4], k[4]]), t0)
    t.same()
    # a set that places a stuck schedule: refused by name, the rest placed
    with pytest.raises(L.CgError) as e:
        d.set([7, 5, 6], t.c_schedules(t.rows([5, 0, 0], [-1, k[1], k[0]])), APIA_T0)
    assert e.value.code == L.CG_ERANGE and "entry 5:" in e.value.msg
    m.set([7, 5, 6], t.rows([5, 0, 0], [-1, never, k[0]]), APIA_T0)
    t.same(skip=[5])
    nx, pv, live = d.snapshot()
    assert nx[5] == NO_PROGRESS and pv[5] == Z and live[5]
    t.remove([5, 7])
    t.same()
    # wakes up to the one whose advance hits the stuck entry
    fired = 0
    while m.effective() != stuck_at:
        assert m.effective() < stuck_at
        t.wake(m.effective())
        fired += 1
    assert fired >= 2 and m.next[1] == m.next[3] == stuck_at
    m.spec[1] = never
    mdue, me = m.fire(stuck_at)
    nd, eff = C.c_int64(), C.c_int64()
    rc, msg = _rc_msg(L.lib().cg_dispatcher_fire(d._h, stuck_at, C.byref(nd), C.byref(eff)))
    assert rc == L.CG_ERANGE and "entry 1:" in msg
    assert nd.value == len(mdue) and mdue.tolist() == [1, 3]
    due = np.empty(nd.value, dtype=np.int32)
    assert L.lib().cg_dispatcher_due(d._h, 0, nd.value, due.ctypes.data) == 0
    _same_array(due, mdue, "due")
    assert eff.value == me == d.effective
    t.same(skip=[1])
    nx, pv, live = d.snapshot()
    assert nx[1] == NO_PROGRESS and pv[1] == stuck_at == m.prev[1] and live[1]
    # it never fires again and never holds the effective time, across the
    # skipped day too
    for _ in range(60):
        assert 1 not in t.wake(m.effective(), snapshot=False)
    t.same(skip=[1])
    t.remove([1])
    t.same()
    for _ in range(3):
        t.wake(m.effective())
    d.free()


# (f) arguments
def test_dispatcher_arguments(eng):
    from cronsun_amd import cron
    L = _lib()
    t = Table("UTC")
    d, m = t.start(eng, t.rows([60, 90, 60], [-1] * 3), T0)

    def refused(code, fn, *a):
        with pytest.raises(L.CgError) as e:
            fn(*a)
        assert e.value.code == code, e.value
        t.same()  # and nothing changed

    refused(L.CG_EINVAL, d.fire, T0 + 59)
    ev = [cron.Every(10**9)]
    refused(L.CG_EINVAL, d.set, [1, 1], ev * 2, T0)
    refused(L.CG_EINVAL, d.set, [2, -1], ev * 2, T0)
    refused(L.CG_EINVAL, d.remove, [3])
    refused(L.CG_EINVAL, d.remove, [0, -1])
    refused(L.CG_ERANGE, d.fire, (1 << 45) + 1)
    refused(L.CG_ERANGE, d.set, [0], ev, -(1 << 45) - 1)
    refused(L.CG_ERANGE, d.set, [0], ev, (1 << 45) + 1)
    with pytest.raises(L.CgError) as e:
        eng.dispatcher(ev, None, (1 << 45) + 1)
    assert e.value.code == L.CG_ERANGE
    assert t.wake(T0 + 60).tolist() == [0, 2]
    out = np.full(4, -7, dtype=np.int32)
    due = L.lib().cg_dispatcher_due
    for first, count in [(-1, 1), (0, 3), (2, 1), (3, 0), (1, -1)]:
        assert due(d._h, first, count, out.ctypes.data) == L.CG_ERANGE, (first, count)
    assert out.tolist() == [-7] * 4
    assert due(d._h, 2, 0, out.ctypes.data) == 0 and due(d._h, 1, 1, out.ctypes.data) == 0
    assert out.tolist() == [2, -7, -7, -7]
    t.remove([0, 1, 2])
    assert d.effective == Z
    due_, e2 = d.fire(T0 + 10**6)
    assert due_.size == 0 and e2 == Z
    t.same()
    d.free()


# (g) the batch kernels past their 4096 x 256 grid, and the SoA upload
N_BATCH = (1 << 20) + 333


@pytest.fixture(scope="module")
def batch_pool():
    """1500 (random_spec | whole-second delay) rows, each with its own
    instant, job kind and AvgTime; the SoA columns of cron.Parse."""
    from cronsun_amd import cron
    rng = np.random.default_rng(1048909)
    p = 1500
    specs = [f"@every {int(rng.integers(1, 7200))}s" if i % 4 == 3 else random_spec(rng)
             for i in range(p)]
    scheds = [cron.Parse(s) for s in specs]
    cols = np.array([[0] * 6 + [s.Delay] if isinstance(s, cron.ConstantDelaySchedule)
                     else [s.Second, s.Minute, s.Hour, s.Dom, s.Month, s.Dow, 0] for s in scheds],
                    dtype=np.uint64)
    t = rng.integers(946684800, 2208988800, p)
    ny = [1772953200, 1793512800, 2099199600, 2119759200]  # 2026 and 2036 transitions
    t[::3] = rng.choice(ny, len(t[::3])) + rng.integers(-86400, 86400, len(t[::3]))
    kind = rng.integers(0, 4, p).astype(np.int32)
    avg = rng.integers(-5000, 20000, p)
    return specs, scheds, oracle_parse_all(specs), cols, t, kind, avg


@pytest.mark.parametrize("zone", ["UTC", "America/New_York"])
def test_batch_kernels_past_grid_cap(eng, batch_pool, zone):
    specs, scheds, osch, cols, t, kind, avg = batch_pool
    oz, z = oracle_zone(zone), product_zone(zone)
    exp_next = np.array([O.sched_next(s, int(x), oz) for s, x in zip(osch, t)], dtype=np.int64)
    exp_ttl = np.array([O.lock_ttl(s, int(x), oz, int(k), int(a), 300)
                        for s, x, k, a in zip(osch, t, kind, avg)], dtype=np.int64)
    ix = np.arange(N_BATCH) % len(specs)
    sp = eng.upload_soa(*[cols[ix, f] for f in range(6)], cols[ix, 6].astype(np.int64))
    assert len(sp) == N_BATCH
    _same_array(eng.next_batch(sp, z, t[ix]), exp_next[ix], "next")
    _same_array(eng.lock_ttl_batch(sp, z, t[ix], kind[ix], avg[ix], 300), exp_ttl[ix], "ttl")
    sp.free()


def test_upload_soa_equals_upload(eng, batch_pool):
    from cronsun_amd import cron
    L = _lib()
    specs, scheds, osch, cols, t, kind, avg = batch_pool
    z = product_zone("America/New_York")
    a = eng.upload(scheds)
    b = eng.upload_soa(*[cols[:, f] for f in range(6)], cols[:, 6].astype(np.int64))
    _same_array(eng.next_batch(b, z, t), eng.next_batch(a, z, t), "next")
    day = 1772953200 - 43200  # across 2026-03-08
    _same_array(eng.count(b, z, day, day + 86400), eng.count(a, z, day, day + 86400), "count")
    # a delay marks an @every row whatever its masks; without one the masks are read
    one = cron.Parse("0 0 * * * *")
    m6 = [[x] * 2 for x in (one.Second, one.Minute, one.Hour, one.Dom, one.Month, one.Dow)]
    c = eng.upload_soa(*m6, [0, 5 * 10**9])
    assert eng.next_batch(c, None, [T0, T0]).tolist() == [T0 + 3600, T0 + 5]
    for bad in (1, 10**9 + 1, 1_500_000_000):
        with pytest.raises(L.CgError) as e:
            eng.upload_soa(*m6, [0, bad])
        assert e.value.code == L.CG_EINVAL
    # a NULL column reads as zero: no second ever matches, as with a zero mask
    zero = [0, 0]
    got = eng.next_batch(eng.upload_soa(None, *m6[1:], zero), None, [T0, T0])
    exp = eng.next_batch(eng.upload_soa(zero, *m6[1:], zero), None, [T0, T0])
    assert got.tolist() == exp.tolist() == [Z, Z]
    for f in range(1, 6):  # each other column alone NULL
        cols_f = [None if g == f else m6[g] for g in range(6)]
        cols_z = [zero if g == f else m6[g] for g in range(6)]
        assert (eng.next_batch(eng.upload_soa(*cols_f, zero), None, [T0, T0]).tolist()
                == eng.next_batch(eng.upload_soa(*cols_z, zero), None, [T0, T0]).tolist())
