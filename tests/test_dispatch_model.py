"""tests/dispatch_model.py pinned on the CPU before it judges the kernels:
against the oracle's Cron.run loop (O.OracleCron) wake by wake, its delay
fast path against its own general path, and three wakes worked by hand."""
import zlib

import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, random_spec
from dispatch_model import DispatchModel, Rows, every

Z = O.ZERO_TIME
LATE = [0, 0, 0, 1, 2, 59, 700, 4000]  # the late-wake choices of test_dispatcher_vs_oracle


def _specs(rng, n):
    """random_spec strings, every fifth an @every"""
    return [f"@every {int(rng.integers(1, 7200))}s" if i % 5 == 4 else random_spec(rng)
            for i in range(n)]


def _same_snapshot(m, oc):
    snap = oc.snapshot()
    assert sorted(snap) == [int(i) for i in np.flatnonzero(m.live)]
    got = {int(i): (int(m.next[i]), int(m.prev[i])) for i in np.flatnonzero(m.live)}
    assert got == snap
    dead = ~m.live
    assert np.all(m.next[dead] == Z) and np.all(m.prev[dead] == Z)


@pytest.mark.parametrize("zone,t0", [
    ("UTC", 1767225600),
    ("America/New_York", 1772953200 - 5400),     # 90 min before 2026-03-08 02:00 EST
    ("Australia/Lord_Howe", 1775314800 - 5400),  # 90 min before the 30-minute fall-back
])
def test_model_vs_oracle_cron(zone, t0):
    rng = np.random.default_rng(zlib.crc32(b"dispatch-model" + zone.encode()))
    n = 300
    osch = oracle_parse_all(_specs(rng, n))
    loc = oracle_zone(zone)
    oc = O.OracleCron(osch, loc)
    oc.start(t0)
    m = DispatchModel(loc, osch)
    m.start(t0)
    _same_snapshot(m, oc)
    next_slot = n
    for w in range(80):
        e = oc.effective()
        assert m.effective() == e, w
        assert e != Z
        now = e + int(rng.choice(LATE))
        due, e2 = m.fire(now)
        assert [int(x) for x in due] == oc.fire(e, now), (w, e, now)
        assert e2 == oc.effective(), w
        _same_snapshot(m, oc)
        if w % 10 == 7:  # add / replace / remove while running
            k = int(rng.integers(1, 6))
            slots = [int(x) for x in rng.choice(next_slot, k, replace=False)]
            if w % 20 == 7:  # extend, once leaving skipped slots
                next_slot += 1 if w != 27 else 4
                slots.append(next_slot - 1)
            new = oracle_parse_all(_specs(rng, len(slots)))
            m.set(slots, new, now)
            for s, osc in zip(slots, new):
                oc.set(s, osc, now)
            rm = [int(x) for x in rng.choice(n, 3, replace=False) if int(x) not in slots]
            m.remove(rm)
            for s in rm:
                oc.remove(s)
            assert m.effective() == oc.effective()
            _same_snapshot(m, oc)
    assert len(m) == next_slot


def test_delay_fast_path_equals_general_path():
    """The same delay-only table as numpy delays and as oracle @every
    schedules: the two paths of the model give the same wakes."""
    rng = np.random.default_rng(7)
    n, t0 = 500, 1767225600
    d = rng.choice([5, 7, 60, 90, 600, 900, 3600], n).astype(np.int64)
    loc = oracle_zone("America/New_York")
    fast = DispatchModel(loc, Rows(d, np.full(n, -1, dtype=np.int32)))
    slow = DispatchModel(loc, [every(x) for x in d])
    assert np.all(fast.spec == -1) and np.all(slow.delay == 0)
    fast.start(t0)
    slow.start(t0)
    for w in range(60):
        e = fast.effective()
        assert e == slow.effective()
        now = e + int(rng.choice(LATE))
        df, ef = fast.fire(now)
        ds, es = slow.fire(now)
        assert np.array_equal(df, ds) and ef == es
        if w % 10 == 3:
            slots = rng.choice(n + 5, 4, replace=False)
            nd = rng.choice([3, 11, 1800], 4).astype(np.int64)
            fast.set(slots, Rows(nd, np.full(4, -1, dtype=np.int32)), now)
            slow.set(slots, [every(x) for x in nd], now)
            rm = rng.choice(n, 2, replace=False)
            fast.remove(rm)
            slow.remove(rm)
        assert np.array_equal(fast.next, slow.next) and np.array_equal(fast.prev, slow.prev)
        assert np.array_equal(fast.live, slow.live)
    assert fast.oracle_calls == 0 and slow.oracle_calls > 0


def test_three_hand_worked_wakes():
    """A 6-slot table in UTC from 2026-01-01 00:00:00: a tie between a delay
    and a spec, a zero-time entry that never fires, and a late wake whose new
    effective time is already past."""
    t0 = 1767225600
    sp = oracle_parse_all(["0 * * * * *", "0 0 0 30 Feb ?", "30 * * * * *", "0 0 * * * *"])
    m = DispatchModel(oracle_zone("UTC"), [60, sp[0], sp[1], 90, sp[2], sp[3]])
    m.start(t0)
    assert m.next.tolist() == [1767225660, 1767225660, Z, 1767225690, 1767225630, 1767229200]
    assert m.prev.tolist() == [Z] * 6
    assert m.effective() == 1767225630

    due, e = m.fire(1767225630)  # on time: slot 4 alone
    assert due.tolist() == [4] and e == 1767225660
    assert m.next.tolist() == [1767225660, 1767225660, Z, 1767225690, 1767225690, 1767229200]
    assert m.prev.tolist() == [Z, Z, Z, Z, 1767225630, Z]

    due, e = m.fire(1767225660)  # the tie: the delay and the every-minute spec
    assert due.tolist() == [0, 1] and e == 1767225690
    assert m.next.tolist() == [1767225720, 1767225720, Z, 1767225690, 1767225690, 1767229200]
    assert m.prev.tolist() == [1767225660, 1767225660, Z, Z, 1767225630, Z]

    due, e = m.fire(1767225735)  # 45 s late: Next counts from now, 00:02:00 was missed
    assert due.tolist() == [3, 4] and e == 1767225720
    assert m.next.tolist() == [1767225720, 1767225720, Z, 1767225825, 1767225750, 1767229200]
    assert m.prev.tolist() == [1767225660, 1767225660, Z, 1767225690, 1767225690, Z]

    due, e = m.fire(1767225735)  # the missed 00:02:00 entries fire next
    assert due.tolist() == [0, 1] and e == 1767225750
    assert m.next.tolist() == [1767225795, 1767225780, Z, 1767225825, 1767225750, 1767229200]

    m.remove([4])
    assert m.effective() == 1767225780 and not m.live[4]
    m.set([7], [5], 1767225740)
    assert len(m) == 8 and m.live.tolist() == [True] * 4 + [False, True, False, True]
    assert m.next[7] == 1767225745 and m.next[6] == Z and m.effective() == 1767225745
    m.remove([0, 1, 3, 5, 7])
    assert m.effective() == Z and m.fire(1767225800)[0].size == 0
