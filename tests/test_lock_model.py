"""The lock model (lock_model.py: the literal fire-by-fire process over the
oracle's expansion) pinned by cases derived by hand, with a stub ttl_of whose
values are worked out in each docstring (and, where the oracle can say, checked
against its lockTtl).  CPU only."""
import numpy as np
import pytest

import lock_model as LM
import oracle_lib as O
import profile_model as PM
from common import oracle_parse_all, oracle_zone

T0 = 1767571217  # 2026-01-05 00:00:17 UTC
C, A, I = LM.COMMON, LM.ALONE, LM.INTERVAL


def lists(specs, horizon, t0=T0):
    return O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + horizon, oracle_zone("UTC"))


def run(specs, w, B, kind, avg_ms, ttl, unit=None, contends=None, t0=T0):
    """(granted, skipped, starts, asked): ttl a constant, a callable or a dict
    {(rule, t): ttl}; asked lists the fires ttl_of was evaluated at."""
    off, times = lists(specs, w * B, t0)
    K = len(specs)
    kind = np.full(K, kind, dtype=np.int32) if np.isscalar(kind) else np.asarray(kind, dtype=np.int32)
    avg = np.full(K, avg_ms, dtype=np.int64) if np.isscalar(avg_ms) else np.asarray(avg_ms, dtype=np.int64)
    asked = []

    def ttl_of(r, t):
        asked.append((r, t))
        if callable(ttl):
            return ttl(r, t)
        return ttl[(r, t)] if isinstance(ttl, dict) else ttl
    g, s = LM.lock_from_lists(off, times, t0, w, B, kind, avg, unit, contends, ttl_of)
    starts = PM.bin_fires(off, times, t0, w, B)
    assert np.array_equal(g + s, starts)
    return g, s, starts, asked


def oracle_ttl(spec, now, kind, avg, lock_ttl=300):
    return O.lock_ttl(oracle_parse_all([spec])[0], now, oracle_zone("UTC"), kind, avg, lock_ttl)


def test_alone_every_60s_2500ms_runs_every_other_minute():
    """@every 60s, ALONE, AvgTime 2500: cost = 2500 / 1000 = 2 (the reference's
    integer slip never rounds up), ttl = 60 - 2 = 58.  The command ends at
    t + 2.5 s, the lease at t + 60.5 s: the fire at t + 60 finds the key, the
    one at t + 120 does not.  Runs at t0 + 60, + 180, ..."""
    assert oracle_ttl("@every 60s", T0 + 60, A, 2500) == 58
    g, s, _, asked = run(["@every 60s"], 60, 10, A, 2500, 58)
    assert g[0].tolist() == [1, 0] * 5 and s[0].tolist() == [0, 1] * 5
    assert [t - T0 for _, t in asked] == [60, 180, 300, 420, 540]  # skipped fires never ask


def test_alone_every_60s_3000ms_runs_every_minute():
    """AvgTime 3000: cost = 3, ttl = 57, the lease ends at t + 3 + 57 = t + 60
    exactly: the next fire is granted."""
    assert oracle_ttl("@every 60s", T0 + 60, A, 3000) == 57
    g, s, starts, _ = run(["@every 60s"], 60, 10, A, 3000, 57)
    assert np.array_equal(g, starts) and not s.any()
    # one ms more and the lease outlives the fire
    g, s, _, _ = run(["@every 60s"], 60, 10, A, 3001, 57)
    assert g[0].tolist() == [1, 0] * 5


def test_interval_hourly_pair_skips_the_second_minute():
    """`0 0,1 * * * *`, INTERVAL: at X:00:00 the next two fires (X:01:00 and
    X+1:00:00) are 3540 s apart, ttl = min(3538, 300) = 300: X:01:00 is skipped
    every hour.  (At X:01:00 the gap would be 60 s, ttl 58 -- never asked.)"""
    t0 = 1767571200 - 30  # 23:59:30
    assert oracle_ttl("0 0,1 * * * *", t0 + 30, I, 0) == 300
    assert oracle_ttl("0 0,1 * * * *", t0 + 30, I, 0, lock_ttl=5000) == 3538
    g, s, _, asked = run(["0 0,1 * * * *"], 60, 180, I, 0, 300, t0=t0)
    assert np.nonzero(g[0])[0].tolist() == [0, 60, 120] and np.nonzero(s[0])[0].tolist() == [1, 61, 121]
    assert len(asked) == 3


def test_two_rule_interval_job_second_rule_never_runs():
    """Rules `0 * * * * *` and `30 * * * * *` of one INTERVAL job: each rule's
    own next two fires are 60 s apart, ttl = 58.  t0 is hh:mm:17, so the :30
    rule fires first (cold start) and holds the key to :28 of the next minute:
    the :00 fire is skipped, the :30 one granted again -- the rule that comes
    first after t0 starves the other.  From t0 at :47 it is the other way."""
    specs = ["0 * * * * *", "30 * * * * *"]
    g, s, starts, _ = run(specs, 60, 10, I, 0, 58, unit=[0, 0])
    assert not g[0].any() and np.array_equal(s[0], starts[0]) and np.array_equal(g[1], starts[1])
    g, s, starts, _ = run(specs, 60, 10, I, 0, 58, unit=[0, 0], t0=T0 + 30)
    assert np.array_equal(g[0], starts[0]) and not g[1].any() and np.array_equal(s[1], starts[1])
    # as jobs of their own nothing is skipped
    g, s, starts, _ = run(specs, 60, 10, I, 0, 58, unit=None)
    assert np.array_equal(g, starts)


def test_same_second_tie_goes_to_the_lower_rule():
    specs = ["0 * * * * *", "0 * * * * *"]
    g, s, starts, asked = run(specs, 60, 10, I, 0, 58, unit=[3, 3])
    assert np.array_equal(g[0], starts[0]) and not s[0].any()
    assert not g[1].any() and np.array_equal(s[1], starts[1])
    assert {r for r, _ in asked} == {0}


def test_ttl_zero_skips_and_leaves_the_state():
    """@every 10s INTERVAL with ttl 25 from the fire at +10, 0 at +40 and 5 at
    +50: +10 granted (key to +35), +20 +30 skipped, +40 free but ttl 0 ->
    skipped with the key still gone, +50 granted (to +55), +60 granted."""
    ttl = {(0, T0 + 10): 25, (0, T0 + 40): 0, (0, T0 + 50): 5, (0, T0 + 60): 100}
    g, s, _, asked = run(["@every 10s"], 10, 6, I, 0, ttl)
    assert g[0].tolist() == [1, 0, 0, 0, 1, 1] and s[0].tolist() == [0, 1, 1, 1, 0, 0]
    assert [t - T0 for _, t in asked] == [10, 40, 50, 60]


def test_non_contending_rule_in_the_middle_of_a_unit():
    """Three every-20-s rules offset by 0, 5 and 10 s in one INTERVAL job, the
    middle one reaching no lock: its row is its start row and it neither takes
    nor finds the key.  ttl 8: rule 0 at :00 holds to :08, rule 2 at :10 to
    :18 -- both always granted; with the middle rule contending (:05 < :08) it
    would be skipped."""
    specs = ["0/20 * * * * *", "5/20 * * * * *", "10/20 * * * * *"]
    g, s, starts, asked = run(specs, 60, 5, I, 0, 8, unit=[0, 0, 0], contends=[1, 0, 1])
    assert np.array_equal(g, starts) and not s.any()
    assert {r for r, _ in asked} == {0, 2}
    g, s, starts, _ = run(specs, 60, 5, I, 0, 8, unit=[0, 0, 0])
    assert np.array_equal(s[1], starts[1]) and not s[0].any() and not s[2].any()
    # no rule contends: the unit is as good as COMMON
    g, s, starts, asked = run(specs, 60, 5, A, 10**9, 8, unit=[0, 0, 0], contends=[0, 0, 0])
    assert np.array_equal(g, starts) and not s.any() and not asked


def test_common_units_are_the_start_profile():
    specs = ["* * * * * *", "@every 7s", "0 * * * * *"]
    g, s, starts, asked = run(specs, 7, 30, C, 3_600_000, 10**6, unit=[0, 0, 1])
    assert np.array_equal(g, starts) and not s.any() and not asked
    # a COMMON unit between two lock units
    g, s, starts, _ = run(specs, 7, 30, [A, C, I], [5000, 5000, 0], 2, unit=None)
    assert np.array_equal(g[1], starts[1]) and s[0].any() and not s[2].any()


@pytest.mark.parametrize("kind,avg,ttl,period", [(I, 10**9, 5, 5), (A, 3000, 2, 5), (A, 2999, 2, 5), (A, -7000, 5, 5),
                                                 (A, 0, 5, 5)])
def test_a_fire_exactly_at_free_at_is_granted(kind, avg, ttl, period):
    """Every-second rule: the lease ends `period` seconds after each grant
    (INTERVAL ignores AvgTime; ALONE adds ceil(max(avg, 0) / 1000)), and the
    fire of that very second is granted."""
    g, s, _, _ = run(["* * * * * *"], 1, 40, kind, avg, ttl)
    assert g[0].tolist() == [int(b % period == 0) for b in range(40)]


def test_one_ms_past_the_second_holds_one_more_fire():
    g, _, _, _ = run(["* * * * * *"], 1, 40, A, 3001, 2)
    assert g[0].tolist() == [int(b % 6 == 0) for b in range(40)]


def test_stuck_and_mixed_units():
    with pytest.raises(LM.LockStuck) as e:
        run(["@every 10s"], 10, 6, I, 0, lambda r, t: None if t == T0 + 30 else 15)
    assert (e.value.rule, e.value.t) == (0, T0 + 30)
    with pytest.raises(AssertionError):
        run(["@every 10s", "@every 10s"], 10, 6, [A, I], 0, 5, unit=[0, 0])
    with pytest.raises(AssertionError):
        run(["@every 10s", "@every 10s"], 10, 6, A, [1, 2], 5, unit=[0, 0])
