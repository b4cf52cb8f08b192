"""The admission model (admit_model.py: the literal fire-by-fire process over
the oracle's expansion) pinned by cases derived by hand.  CPU only."""
import numpy as np
import pytest

import admit_model as AM
import oracle_lib as O
import profile_model as PM
from common import oracle_parse_all, oracle_zone

T0 = 1767571217  # 2026-01-05 00:00:17 UTC


def lists(specs, horizon, t0=T0, zone="UTC"):
    return O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + horizon, oracle_zone(zone))


def admit(specs, w, B, dur_ms, parallels, unit=None, t0=T0):
    off, times = lists(specs, w * B, t0)
    K = len(specs)
    dur = np.full(K, dur_ms, dtype=np.int64) if np.isscalar(dur_ms) else np.asarray(dur_ms, dtype=np.int64)
    par = np.full(K, parallels, dtype=np.int64) if np.isscalar(parallels) else np.asarray(parallels, dtype=np.int64)
    adm, drop = AM.admit_from_lists(off, times, t0, w, B, dur, par, unit)
    starts = PM.bin_fires(off, times, t0, w, B)
    assert np.array_equal(adm + drop, starts)
    return adm, drop, starts


def test_every_second_ten_second_runs():
    """`* * * * * *` running 10 s: P = 1 admits one fire per 10 s (the one at
    the very second the previous instance ends), P = 2 two."""
    adm, drop, _ = admit(["* * * * * *"], 1, 60, 10_000, 1)
    assert adm[0].tolist() == [int(b % 10 == 0) for b in range(60)]
    assert drop[0].tolist() == [int(b % 10 != 0) for b in range(60)]
    adm, drop, _ = admit(["* * * * * *"], 1, 60, 10_000, 2)
    assert adm[0].tolist() == [int(b % 10 < 2) for b in range(60)]
    # in 10-s buckets: 1 (2) admitted and 9 (8) dropped per bucket
    adm, drop, _ = admit(["* * * * * *"], 10, 6, 10_000, 1)
    assert adm[0].tolist() == [1] * 6 and drop[0].tolist() == [9] * 6
    adm, drop, _ = admit(["* * * * * *"], 10, 6, 10_000, 2)
    assert adm[0].tolist() == [2] * 6 and drop[0].tolist() == [8] * 6


def test_every_7s_running_20s_admits_every_third_fire():
    """@every 7s fires at t0 + 7, 14, 21, ...: the run from +7 ends at +27, so
    +14 and +21 are dropped and +28 is admitted."""
    adm, drop, _ = admit(["@every 7s"], 1, 84, 20_000, 1)
    fires = [7 * k for k in range(1, 13)]
    assert np.nonzero(adm[0])[0].tolist() == [t - 1 for t in fires[0::3]]
    assert np.nonzero(drop[0])[0].tolist() == [t - 1 for t in fires if (t // 7 - 1) % 3]


@pytest.mark.parametrize("ms,admitted", [(999, 40), (1000, 40), (1001, 20)])
def test_around_one_second(ms, admitted):
    """Against a 1-s period: 999 ms and 1000 ms have ended when the next fire
    comes (a * 1000 + 1000 > (a + 1) * 1000 is false), 1001 ms has not."""
    adm, drop, _ = admit(["* * * * * *"], 1, 40, ms, 1)
    assert int(adm.sum()) == admitted and int(drop.sum()) == 40 - admitted
    if ms == 1001:
        assert adm[0].tolist() == [1, 0] * 20


def test_lower_rule_wins_the_second():
    """Two rules of one unit firing in the same seconds, P = 1, 30-s runs: the
    lower rule is admitted every time, the higher never; as units of their
    own both are admitted."""
    specs = ["0 * * * * *", "0 * * * * *"]
    adm, drop, starts = admit(specs, 60, 10, 30_000, 1, unit=[4, 4])
    assert np.array_equal(adm[0], starts[0]) and not drop[0].any()
    assert np.array_equal(drop[1], starts[1]) and not adm[1].any()
    adm, drop, starts = admit(specs, 60, 10, 30_000, 1, unit=None)
    assert np.array_equal(adm, starts) and not drop.any()
    # P = 2: both fit
    adm, drop, starts = admit(specs, 60, 10, 30_000, 2, unit=[0, 0])
    assert np.array_equal(adm, starts)


def test_unit_shares_one_limit_across_rules():
    """Rules at :00 and :20 of every minute in one unit, 30-s runs, P = 1: the
    :20 fire finds the :00 instance running and is dropped -- but for the very
    first one (t0 is hh:mm:17, so :20 comes first and nothing is known to
    run: the cold start)."""
    adm, drop, starts = admit(["0 * * * * *", "20 * * * * *"], 60, 10, 30_000, 1, unit=[0, 0])
    assert np.array_equal(adm[0], starts[0]) and not drop[0].any()
    assert adm[1].tolist() == [1] + [0] * 9 and drop[1].tolist() == [0] + [1] * 9


@pytest.mark.parametrize("P,ms", [(0, 3_600_000), (1, 0), (3, 0), (2, 2000), (2, 1001), (10, 5000), (16, 1)])
def test_units_that_never_drop_equal_the_starts(P, ms):
    """P = 0, d = 0 and P >= k * d (here k = 2 rules firing every second, in
    one unit only where P >= 2 d)."""
    specs = ["* * * * * *", "* * * * * *", "@every 3s"]
    d = -(-ms // 1000)
    unit = [0, 0, 1] if AM.never_drops(P, d, 2) else None
    assert AM.never_drops(P, d, 2 if unit else 1)
    adm, drop, starts = admit(specs, 7, 30, ms, P, unit=unit)
    assert np.array_equal(adm, starts) and not drop.any()


def test_admitted_plus_dropped_is_the_start_profile():
    """A seeded mix in units of 1 to 5 rules with P in {0, 1, 2, 16} and
    durations from none to past the horizon."""
    rng = np.random.default_rng(12)
    pool = ["* * * * * *", "*/7 * * * * *", "@every 11s", "0 */5 * * * *", "7,30,45 * * * * *", "@every 90s",
            "0 0 0 30 Feb ?", "*/20 */2 * * * *"]
    specs = [pool[i] for i in rng.integers(0, len(pool), 40)]
    sizes, unit = [], []
    while len(unit) < len(specs):
        k = min(int(rng.integers(1, 6)), len(specs) - len(unit))
        unit += [len(sizes)] * k
        sizes.append(k)
    dur_u = rng.choice([0, 1, 999, 1001, 10_000, 60_000, 3_600_000, (1 << 63) - 1], len(sizes))
    par_u = rng.choice([0, 1, 2, 16], len(sizes))
    dur, par = np.repeat(dur_u, sizes), np.repeat(par_u, sizes)
    adm, drop, starts = admit(specs, 37, 50, dur, par, unit=unit)
    assert drop.any() and adm.any() and (drop >= 0).all() and (adm >= 0).all()
    for u, k in enumerate(sizes):
        rows = [r for r in range(len(specs)) if unit[r] == u]
        if par_u[u] == 0 or dur_u[u] == 0:
            assert not drop[rows].any()
        elif par_u[u] <= 2 and dur_u[u] >= 3_600_000:  # the whole horizon: only the first P fires run
            assert int(adm[rows].sum()) == min(int(par_u[u]), int(starts[rows].sum()))


def test_units_of():
    assert AM.units_of(None, 3) == [(0, 1), (1, 2), (2, 3)]
    assert AM.units_of([5, 5, 7, 9, 9, 9], 6) == [(0, 2), (2, 3), (3, 6)]
    assert AM.units_of([], 0) == []
    with pytest.raises(AssertionError):
        AM.units_of([1, 0], 2)
    with pytest.raises(AssertionError):  # mixed values inside a unit
        admit(["* * * * * *", "* * * * * *"], 1, 5, [1000, 2000], 1, unit=[0, 0])
