"""Pipelined expansions on two writer streams and two output buffers
(cg_expand_device_async with cg_set_async_overlap on, the default) and on one
(off): every result bit-exact against the synchronous cg_expand_device of the
same window on the same engine, which the other suites pin to the oracle."""
import time

import numpy as np
import pytest

from common import product_zone
from cronsun_amd import _lib, cron, synth
from cronsun_amd._lib import check, lib

pytestmark = pytest.mark.gpu

DAY = 86400
SPRING_2026 = 1772953200  # America/New_York, 2026-03-08 02:00 EST -> 03:00 EDT
LENGTHS = (DAY, 60, 3600)  # position slices, cost-space slices, ...; long writer before a short one


def make_engine(overlap, n_rules, seed):
    from cronsun_amd.engine import Engine
    eng = Engine(0)
    if not overlap:
        eng.set_async_overlap(0)
    specs = synth.spec_mix(n_rules, seed=seed)
    arr, status = cron.parse_batch(specs)
    assert (status == 0).all()
    return eng, eng.upload_c(arr, n_rules), n_rules


def read_result(eng, R, E):
    off = np.empty(R + 1, dtype=np.int64)
    check(lib().cg_result_copy_offsets(eng._h, off.ctypes.data))
    return E, off, eng.copy_times(0, E)


def sync_result(eng, sp, R, zone, a, b):
    return read_result(eng, R, eng.expand_device(sp, zone, a, b))


def assert_same(got, want, what):
    assert got[0] == want[0], what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what


def run_batch(eng, sp, R, zone, wins):
    """the windows pipelined, one wait; the last one's result against its
    synchronous expansion (made afterwards: it writes the first buffer)"""
    for a, b in wins:
        eng.expand_async(sp, zone, a, b)
    got = read_result(eng, R, eng.expand_wait())
    assert_same(got, sync_result(eng, sp, R, zone, *wins[-1]), wins[-1])
    return got


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("zone", ["UTC", "America/New_York"])
def test_every_position_is_last_once(zone, overlap):
    """Batches of 1, 2, 3, 4, 5 and 8 calls (odd and even lengths: both buffers
    end up last; more than three: the run sets are reused), T0 moving every
    call and the window length alternating 24 h, 60 s, 1 h, so a long writer
    is followed by one that ends in a fraction of its time.  In New York the
    24-h windows hold the 2026 spring-forward: the walk writer runs behind
    k_write_cf, on either writer stream."""
    eng, sp, R = make_engine(overlap, 10_000, seed=21)
    z = product_zone(zone)
    t0 = SPRING_2026 - 12 * 3600
    eng.expand_device(sp, z, t0, t0 + 3 * DAY)  # sizes the output
    call = 0
    for n in (1, 2, 3, 4, 5, 8):
        wins = []
        for j in range(n):
            a = t0 + 1800 * call + 7 * j
            wins.append((a, a + LENGTHS[j % 3]))
            call += 1
        run_batch(eng, sp, R, z, wins)
    sp.free()
    eng.close()


@pytest.mark.parametrize("overlap", [1, 0])
def test_no_stale_or_unwritten_words(overlap):
    """Both output buffers poisoned over their whole capacity, then a batch of
    four moving 24-h windows: no poisoned word is left inside the result."""
    eng, sp, R = make_engine(overlap, 20_000, seed=22)
    t0 = synth.T0_2026
    cap = eng.expand_device(sp, None, t0, t0 + 3 * DAY)  # the first call sizes the output to its events
    ptrs = []
    for i in range(2):
        eng.expand_async(sp, None, t0 + i, t0 + i + DAY)
        eng.expand_wait()
        ptrs.append(eng.result_device()[1])
    if overlap:
        assert ptrs[0] != ptrs[1]  # the documented behaviour where the second buffer fits
    else:
        assert ptrs[0] == ptrs[1]
    for p in set(ptrs):
        eng.fill(p, cap * 8, 0xFF)
    wins = [(t0 + 600 * i, t0 + 600 * i + DAY) for i in range(4)]
    for a, b in wins:
        eng.expand_async(sp, None, a, b)
    E = eng.expand_wait()
    _, d_times, n = eng.result_device()
    assert n == E and d_times in ptrs
    assert eng.count_value(d_times, E, 8, -1) == 0
    got = read_result(eng, R, E)
    assert_same(got, sync_result(eng, sp, R, None, *wins[-1]), "poisoned buffers")
    sp.free()
    eng.close()


@pytest.mark.parametrize("overlap", [1, 0])
def test_error_in_the_middle(overlap):
    """The third of five calls exceeds the capacity: the wait reports
    CG_ECAPACITY; both buffers and all run sets serve the next batch."""
    eng, sp, R = make_engine(overlap, 5_000, seed=23)
    t0 = synth.T0_2026
    eng.expand_device(sp, None, t0, t0 + 3 * DAY)
    for i in range(5):
        a = t0 + 900 * i
        eng.expand_async(sp, None, a, a + (30 * DAY if i == 2 else DAY))
    with pytest.raises(_lib.CgError) as err:
        eng.expand_wait()
    assert err.value.code == _lib.CG_ECAPACITY
    run_batch(eng, sp, R, None, [(t0 + 7000 + 900 * i, t0 + 7000 + 900 * i + LENGTHS[i % 3]) for i in range(3)])
    sp.free()
    eng.close()


@pytest.mark.parametrize("overlap", [1, 0])
def test_growth_and_setter(overlap):
    """A synchronous call over a horizon four times longer grows the output:
    the next pipelined batch of windows of that length is correct (the second
    buffer regrown, the slice map built for the new capacity).  The setter
    switches between the paths with nothing pending and is refused otherwise."""
    eng, sp, R = make_engine(overlap, 8_000, seed=24)
    t0 = synth.T0_2026
    eng.expand_device(sp, None, t0, t0 + DAY)
    run_batch(eng, sp, R, None, [(t0 + 60 * i, t0 + 60 * i + DAY - 3600) for i in range(3)])
    E1 = eng.expand_device(sp, None, t0, t0 + DAY)
    E4 = eng.expand_device(sp, None, t0 + 5, t0 + 5 + 4 * DAY)
    assert E4 > 3 * E1
    got = run_batch(eng, sp, R, None, [(t0 + 300 * i, t0 + 300 * i + 4 * DAY - 600) for i in range(3)])
    assert got[0] > E1  # more than the first capacity held
    for on in (0, 1):
        eng.set_async_overlap(on)
        run_batch(eng, sp, R, None, [(t0 + 11 * i + on, t0 + 11 * i + on + LENGTHS[i % 3]) for i in range(4)])
    eng.expand_async(sp, None, t0, t0 + DAY)
    with pytest.raises(_lib.CgError) as err:
        eng.set_async_overlap(1 - overlap)
    assert err.value.code == _lib.CG_EINVAL
    eng.expand_wait()
    sp.free()
    eng.close()


@pytest.mark.parametrize("overlap", [1, 0])
def test_writer_time_is_sane(overlap):
    """kernel_times()[3] after a batch is the mean of per-call writer intervals
    that do not overlap, so n times it cannot exceed the wall time from the
    first enqueue to the wait's return (a bound by construction)."""
    eng, sp, R = make_engine(overlap, 20_000, seed=25)
    t0 = synth.T0_2026
    eng.expand_device(sp, None, t0, t0 + 2 * DAY)
    for i in range(3):  # every run set allocates outside the measured batch
        eng.expand_async(sp, None, t0 + i, t0 + i + DAY)
    eng.expand_wait()
    n = 8
    start = time.perf_counter()
    for i in range(n):
        eng.expand_async(sp, None, t0 + 60 * i, t0 + 60 * i + DAY)
    eng.expand_wait()
    wall_ms = (time.perf_counter() - start) * 1e3
    w = eng.kernel_times()[3]
    print(f"overlap {overlap}: writer {w:.4f} ms x {n} = {n * w:.4f} ms, wall {wall_ms:.4f} ms")
    assert w > 0
    assert n * w <= wall_ms
    sp.free()
    eng.close()
