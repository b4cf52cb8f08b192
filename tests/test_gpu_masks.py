"""The expansion, Next and profile kernels on the rule sets of
tests/mask_cases.py: random second, minute and hour masks of every popcount
(the writer's mixed-radix digits, rank tables, progression test and per-lane
seek, cg_write.h; the profile's partial-mask ranks, cg_profile.h) and the edge
patterns of every level.  Everything is bit-exact against the oracle, which
parses the spec strings itself; tests/test_mask_cases.py checks on the CPU that
the sets hold what they promise."""
import time

import numpy as np
import pytest

import mask_cases as M
import oracle_lib as O
import profile_model as PM
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import cron, synth
from cronsun_amd._lib import check, lib
from test_gpu_expand import check_same

pytestmark = pytest.mark.gpu

DAY = 86400
T0 = synth.T0_2026  # a UTC midnight (a Monday)
UTC_DAY = (T0 + 1234, T0 + DAY)
NY_SPRING, NY_FALL = 1772953200, 1793512800  # 2026-03-08 07:00Z, 2026-11-01 06:00Z
LORD_HOWE_TAU = 1775314800                   # 2026-04-04 15:00Z
SEED = 1


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def fresh():
    from cronsun_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_specs = {}


def day_specs():
    """stratified(360) + extremes(): (specs, product schedules, oracle schedules)"""
    if "day" not in _specs:
        specs = M.stratified(360, SEED) + M.extremes()
        _specs["day"] = specs, [cron.Parse(s) for s in specs], O.sched_array(oracle_parse_all(specs))
    return _specs["day"]


_oracle = {}


def oracle_day(zone, t0, t1):
    """the oracle's CSR of day_specs() over (t0, t1], computed once"""
    if (zone, t0, t1) not in _oracle:
        _oracle[(zone, t0, t1)] = O.expand_batch(day_specs()[2], t0, t1, oracle_zone(zone), threads=16)
    return _oracle[(zone, t0, t1)]


def oracle_in_parts(specs, zone, t0, t1, parts=16):
    """The oracle's CSR of specs, one thread per `parts`-th of the rules.  (Its
    own threads take 64 rules at a time, so 250 sparse rules over 40 days --
    where a Next walks many seconds and minutes per fire -- would keep four
    busy.)  A rule whose reference loop never ends raises O.NonTerminating."""
    from concurrent.futures import ThreadPoolExecutor
    scheds = oracle_parse_all(specs)
    step = -(-len(scheds) // parts)
    chunks = [scheds[i:i + step] for i in range(0, len(scheds), step)]
    oz = oracle_zone(zone)
    with ThreadPoolExecutor(parts) as pool:
        csrs = list(pool.map(lambda c: O.expand_batch(O.sched_array(c), t0, t1, oz, threads=1), chunks))
    counts = np.concatenate([np.diff(o) for o, _ in csrs])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return off, np.concatenate([t for _, t in csrs])


def same_csr(got, want, specs, what):
    """array_equal on offsets and times, naming the first differing rule and index"""
    (off, times), (eo, et) = got, want
    if not np.array_equal(off, eo):
        r = int(np.nonzero(np.diff(off) != np.diff(eo))[0][0])
        raise AssertionError(f"{what}: rule {r} [{specs[r]}] has {int(off[r + 1] - off[r])} fires, "
                             f"not {int(eo[r + 1] - eo[r])}")
    if not np.array_equal(times, et):
        bad = np.nonzero(times != et)[0]
        i = int(bad[0])
        r = int(np.searchsorted(eo, i, side="right") - 1)
        raise AssertionError(f"{what}: {bad.size} of {et.size} times differ; the first at index {i} (fire "
                             f"{i - int(eo[r])} of rule {r} [{specs[r]}], lane {i % 64}): {int(times[i])}, not {int(et[i])}")


def read_result(eng, R, E):
    off = np.empty(R + 1, dtype=np.int64)
    check(lib().cg_result_copy_offsets(eng._h, off.ctypes.data))
    return off, eng.copy_times(0, E)


def report(what, events, t_start):
    print(f"[masks] {what}: {events} events compared, {time.time() - t_start:.1f} s")


@pytest.mark.parametrize("zone,t0,t1", [
    ("UTC",) + UTC_DAY,
    ("America/New_York", NY_SPRING - DAY // 2 - 17, NY_SPRING + DAY // 2),
    ("America/New_York", NY_FALL - DAY // 2 - 17, NY_FALL + DAY // 2),
    ("Australia/Lord_Howe", LORD_HOWE_TAU - DAY // 2 - 17, LORD_HOWE_TAU + DAY // 2)],
    ids=["utc-day", "ny-spring", "ny-fall", "lord-howe"])
def test_whole_csr(eng, zone, t0, t1):
    """One day in UTC from a midnight + 1234 s; the 24 h around New York's 2026
    transitions and Lord Howe's 30-minute one (closed-form and walked runs)."""
    ts = time.time()
    specs, scheds, _ = day_specs()
    if zone != "UTC":
        z = oracle_zone(zone)
        assert z.lookup(t0)[0] != z.lookup(t1)[0]
    off, _ = check_same(eng, scheds, zone, t0, t1, specs)
    report(f"whole CSR {zone} ({t0}, {t1}]", int(off[-1]), ts)


@pytest.mark.parametrize("zone", ["UTC", "America/New_York"])
def test_long_horizon_day_tables(eng, zone):
    """40 days from a midnight - 77 s: a month end and a 31-day segment cut, so
    the matching days of the dom, dow and month lists are a table."""
    ts = time.time()
    specs = M.stratified(240, SEED, sparse=True) + M.day_extremes(sparse=True)
    t0, t1 = T0 - 77, T0 + 40 * DAY
    want = oracle_in_parts(specs, zone, t0, t1)
    got = eng.expand([cron.Parse(s) for s in specs], product_zone(zone), t0, t1)
    same_csr(got, want, specs, f"40 days {zone}")
    assert want[0][-1] > 1_000_000
    report(f"40 days {zone}", int(want[0][-1]), ts)


@pytest.mark.parametrize("width", [60, 3600])
def test_short_windows_after_a_day(eng, width):
    """Short windows right after the day call grew the output: cost-space
    slices at the smallest shifts, mostly per-lane seeks."""
    ts = time.time()
    specs, scheds, oarr = day_specs()
    sp = eng.upload(scheds)
    eng.expand_device(sp, None, *UTC_DAY)
    t0 = T0 + 7 * 3600 + 37
    E = eng.expand_device(sp, None, t0, t0 + width)
    want = O.expand_batch(oarr, t0, t0 + width, oracle_zone("UTC"), threads=16)
    same_csr(read_result(eng, len(specs), E), want, specs, f"{width}-s window")
    assert E > 0
    sp.free()
    report(f"{width}-s window", E, ts)


def test_position_slices(fresh):
    """E >= 2^25: the writer's 2048-event position slices (u_mode off), on
    stratified sets of several seeds over one UTC day."""
    ts = time.time()
    # a set of 360 fires about 3.7 M times that day: ten sets pass 2^25
    specs = [s for seed in range(100, 110) for s in M.stratified(360, seed)]
    want = O.expand_batch(O.sched_array(oracle_parse_all(specs)), *UTC_DAY, oracle_zone("UTC"), threads=16)
    E = int(want[0][-1])
    assert E >> 11 >= 16384  # cg_kernels.h u_mode: position slices, not cost-space ones
    arr, status = cron.parse_batch(specs)
    assert (status == 0).all()
    sp = fresh.upload_c(arr, len(specs))
    for what in ("first call", "second call"):  # slice map by k_chunk_map, then by the scan
        got_E = fresh.expand_device(sp, None, *UTC_DAY)
        assert got_E == E and got_E >> 11 >= 16384
        same_csr(read_result(fresh, len(specs), E), want, specs, f"position slices, {what}")
    sp.free()
    report(f"position slices ({len(specs)} rules, twice)", E, ts)


def test_pipelined(fresh):
    """The UTC day through three pipelined calls with shifted starts, both
    output buffers poisoned first: the last result is the oracle's and no
    word of [0, E) is left unwritten."""
    ts = time.time()
    specs, scheds, _ = day_specs()
    want = oracle_day("UTC", *UTC_DAY)
    t0, t1 = UTC_DAY
    sp = fresh.upload(scheds)
    cap = fresh.expand_device(sp, None, t0, t1 + 600)  # sizes the output
    ptrs = set()
    for i in range(2):
        fresh.expand_async(sp, None, t0 + i, t1 + i)
        fresh.expand_wait()
        ptrs.add(fresh.result_device()[1])
    assert len(ptrs) == 2
    for p in ptrs:
        fresh.fill(p, cap * 8, 0xFF)
    for dt in (7, 3, 0):
        fresh.expand_async(sp, None, t0 + dt, t1 + dt)
    E = fresh.expand_wait()
    assert E == int(want[0][-1]) and E <= cap
    d_times = fresh.result_device()[1]
    assert d_times in ptrs
    assert fresh.count_value(d_times, E, 8, -1) == 0
    same_csr(read_result(fresh, len(specs), E), want, specs, "pipelined")
    sp.free()
    report("pipelined", E, ts)


def _transitions(zone):
    from test_zone import _table
    return _table(product_zone(zone), 946684800, 2208988800)[0][1:]


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Australia/Lord_Howe", "Pacific/Chatham"])
def test_next_batch(eng, zone):
    """Next from instants uniform in 2000-2040, exactly on a fire and one second
    before and after it, at hh:59:59 and 23:59:59 local, and within a day of a
    transition: the walk's jumps to the next set bit over arbitrary gaps."""
    ts = time.time()
    specs, scheds, oarr = day_specs()
    n = len(specs)
    oz, z = oracle_zone(zone), product_zone(zone)
    rng = np.random.default_rng(sum(zone.encode()))
    uniform = rng.integers(946684800, 2208988800, n)
    batches = {"uniform": uniform}
    day = (NY_FALL - DAY // 2 - 17, NY_FALL + DAY // 2 - 17) if zone == "America/New_York" else UTC_DAY
    eo, et = oracle_day(zone, *day)  # (the windows of the profile and pipelined tests: one oracle run each)
    cnt = np.diff(eo)
    pick = eo[:-1] + (rng.integers(0, 1 << 30, n) % np.maximum(cnt, 1))
    fire = np.where(cnt > 0, et[np.minimum(pick, et.size - 1)], uniform)  # no fire that day: a uniform instant
    batches.update({"on a fire": fire, "fire - 1": fire - 1, "fire + 1": fire + 1})
    u = rng.integers(946684800, 2208988800, n)
    local = u + np.array([oz.lookup(int(x))[0] for x in u])
    batches["hh:59:59"] = u - local % 3600 + 3599
    u = rng.integers(946684800, 2208988800, n)
    local = u + np.array([oz.lookup(int(x))[0] for x in u])
    batches["23:59:59"] = u - local % DAY + DAY - 1
    when = _transitions(zone)
    if len(when):
        batches["near a transition"] = when[rng.integers(0, len(when), n)] + rng.integers(-DAY, DAY, n)
    sp = eng.upload(scheds)
    for what, t in batches.items():
        t = np.ascontiguousarray(t, dtype=np.int64)
        if what in ("hh:59:59", "23:59:59"):  # (a few instants next to a transition may be off: most must hold)
            loc = t + np.array([oz.lookup(int(x))[0] for x in t])
            assert (loc % (3600 if what[0] == "h" else DAY) == (3599 if what[0] == "h" else DAY - 1)).mean() > 0.99
        got = eng.next_batch(sp, z, t)
        exp = np.array([O.sched_next(oarr[i], int(t[i]), oz) for i in range(n)], dtype=np.int64)
        if not np.array_equal(got, exp):
            i = int(np.nonzero(got != exp)[0][0])
            raise AssertionError(f"{zone} {what}: rule {i} [{specs[i]}] Next({int(t[i])}) = {int(got[i])}, not {int(exp[i])}")
    sp.free()
    report(f"next_batch {zone} ({len(batches)} batches)", n * len(batches), ts)


@pytest.mark.parametrize("zone,t0", [("UTC", UTC_DAY[0]), ("America/New_York", NY_FALL - DAY // 2 - 17)],
                         ids=["utc", "ny-fall"])
def test_fire_profile(eng, zone, t0):
    """The rule matrix at widths 1, 7, 61 and 3599 s (an hour up to a day of
    buckets): the edges fall inside minutes and hours, so the ranks are taken
    on partial masks, at s = 59, m = 59 and h = 23 too; the New York day holds
    the fall-back (walked runs)."""
    ts = time.time()
    specs, scheds, _ = day_specs()
    eo, et = oracle_day(zone, t0, t0 + DAY)
    sp = eng.upload(scheds)
    z = product_zone(zone)
    events = 0
    for w, B in ((1, 3600), (7, 4096), (61, 1416), (3599, 24)):
        assert 3600 <= w * B <= DAY
        exp = PM.bin_fires(eo, et, t0, w, B)
        got, totals = eng.profile(sp, z, t0, w, B)
        if not np.array_equal(got, exp):
            r, b = [int(x[0]) for x in np.nonzero(got != exp)]
            raise AssertionError(f"{zone} w={w} B={B}: rule {r} [{specs[r]}] bucket {b}: {int(got[r, b])}, not {int(exp[r, b])}")
        assert np.array_equal(totals, exp.sum(axis=0, dtype=np.int64))
        events += int(exp.sum(dtype=np.int64))
    sp.free()
    report(f"fire profile {zone}", events, ts)


def test_junk_bits(eng):
    """Bits the reference never looks at (second and minute 60-62, hour 24-62,
    dom 0 and 32-62, month 0 and 13-62, dow 7-62) change nothing."""
    ts = time.time()
    specs = day_specs()[0]
    cols = M.soa_columns(specs)
    junk = M.junk_bits(cols, 7)
    assert any(not np.array_equal(a, b) for a, b in zip(cols, junk))
    zero = np.zeros(len(specs), dtype=np.int64)
    want = oracle_day("UTC", *UTC_DAY)
    clean = eng.expand(eng.upload_soa(*cols, zero), None, *UTC_DAY)
    same_csr(clean, want, specs, "clean columns")
    dirty = eng.expand(eng.upload_soa(*junk, zero), None, *UTC_DAY)
    assert np.array_equal(dirty[0], clean[0]) and np.array_equal(dirty[1], clean[1])
    report("junk bits", 2 * int(want[0][-1]), ts)
