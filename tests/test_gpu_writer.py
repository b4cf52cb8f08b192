"""The closed-form writer (k_write_cf, cg_write.h) on the constructed rule
sets of tests/writer_cases.py: the whole rule-major CSR bit-exact against the
oracle in every slice mode the writer has below a capacity of 2^31 events
(cost-space slices of about 64 events, cost-space slices at larger shifts,
2048-event position slices mapped by k_chunk_map and by the scan, the sizes
around the switch between the modes), synchronously and pipelined, and the
words of the output buffer past E left alone.  tests/test_writer_cases.py
checks on the CPU that the sets hold the cases they promise."""
import numpy as np
import pytest

import oracle_lib as O
import writer_cases as W
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import cron
from cronsun_amd._lib import check, lib

pytestmark = pytest.mark.gpu


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


def oracle_csr(case):
    arr = O.sched_array(oracle_parse_all(case.specs))
    eo, et = O.expand_batch(arr, case.t0, case.t1, oracle_zone(case.zone), threads=16)
    assert np.array_equal(eo, case.off), case.name  # the builder placed its runs where it says
    return eo, et


def upload(eng, case):
    arr, status = cron.parse_batch(case.specs)
    assert (status == 0).all()
    return eng.upload_c(arr, len(case.specs))


def read_result(eng, R, E):
    off = np.empty(R + 1, dtype=np.int64)
    check(lib().cg_result_copy_offsets(eng._h, off.ctypes.data))
    return off, eng.copy_times(0, E)


def expand(eng, sp, case, dt=0, longer=0):
    return eng.expand_device(sp, product_zone(case.zone), case.t0 + dt, case.t1 + dt + longer)


def assert_csr(case, got, want, what):
    """bit-exact, naming the first rule that differs"""
    (off, times), (eo, et) = got, want
    if not np.array_equal(off, eo):
        r = int(np.nonzero(np.diff(off) != np.diff(eo))[0][0])
        raise AssertionError(f"{case.name} {what}: {int(off[r + 1] - off[r])} fires, not {int(eo[r + 1] - eo[r])}, "
                             f"for {W.describe(case, r)}")
    if not np.array_equal(times, et):
        bad = np.nonzero(times != et)[0]
        i = int(bad[0])
        r = int(np.searchsorted(eo, i, side="right") - 1)
        rules = np.unique(np.searchsorted(eo, bad, side="right") - 1)
        forms = sorted({W.FORMS[case.ledger.form[k]] for k in rules})
        raise AssertionError(
            f"{case.name} {what}: {bad.size} of {et.size} times differ in {rules.size} rules (forms {forms}); the first at "
            f"index {i} (fire {i - int(eo[r])} of its run, lane {i % 64} of its block, slice {i // W.SLICE}): "
            f"{int(times[i])}, not {int(et[i])}, for {W.describe(case, r)}")


def check_same(eng, sp, case, want, what):
    E = expand(eng, sp, case)
    assert E == int(want[0][-1]), (case.name, what)
    assert_csr(case, read_result(eng, len(case.specs), E), want, what)
    return E


def poison(eng, cap):
    """the last result's buffer filled with -1 over the capacity known to the test"""
    ptr = eng.result_device()[1]
    eng.fill(ptr, cap * 8, 0xFF)
    return ptr


def check_guard(eng, E, cap, ptrs, what):
    """no -1 left inside [0, E) of the last result, every word of [E, cap) still -1"""
    _, d_times, n = eng.result_device()
    assert n == E and d_times in ptrs, what
    assert cap > E, what
    left = eng.count_value(d_times, E, 8, -1)
    kept = eng.count_value(d_times + 8 * E, cap - E, 8, -1)
    assert left == 0, f"{what}: {left} words of [0, {E}) unwritten"
    assert kept == cap - E, f"{what}: {cap - E - kept} of the {cap - E} words past E = {E} overwritten"


def steady_state(eng, sp, case, want, what, cap=None):
    """A call on a buffer sized by a larger call (when cap is not given yet: the
    same window 600 s longer) and poisoned: the whole CSR and the guard words.
    Returns (cap, E)."""
    if cap is None:
        cap = expand(eng, sp, case, longer=600)
    ptr = poison(eng, cap)
    E = check_same(eng, sp, case, want, what)
    check_guard(eng, E, cap, {ptr}, what)
    return cap, E


def pipelined(eng, sp, case, cap, E, checksum, what):
    """Both output buffers poisoned, then the window pipelined three times (its
    start moved by 0, 7 and 0 s), and again twice (7 and 0 s): the last
    result's checksum and guard words, on two writer streams and on one."""
    z = product_zone(case.zone)
    for overlap in (1, 0):
        eng.set_async_overlap(overlap)
        ptrs = set()
        for i in range(2):  # one call into either buffer
            eng.expand_async(sp, z, case.t0 + i, case.t1 + i)
            eng.expand_wait()
            ptrs.add(eng.result_device()[1])
        assert len(ptrs) == (2 if overlap else 1)
        # with two buffers the third call writes where the first one wrote the
        # same window; after (7, 0) the last call's buffer held nothing but poison
        for moves in ((0, 7, 0), (7, 0)):
            for p in ptrs:
                eng.fill(p, cap * 8, 0xFF)
            for dt in moves:
                eng.expand_async(sp, z, case.t0 + dt, case.t1 + dt)
            assert eng.expand_wait() == E
            w = f"{what}, pipelined {moves}, overlap {overlap}"
            check_guard(eng, E, cap, ptrs, w)
            assert eng.checksum(eng.result_device()[1], E) == checksum, w
    eng.set_async_overlap(1)


def test_sweep_alignments_and_lengths(eng):
    """Every generator of the sweep at the start residues 0, 1, 31, 32, 33, 62
    and 63 mod 64 and at 23 lengths around 1, 64, 128, 512, 576, 640, 2048 and
    2112, where the cost shift is 6: a slice is at most one 64-event block, so
    there is a cut inside almost every run, every piece seeds its digits
    afresh at its own offset into the run, and blocks are shared by several
    runs.  (No piece is stepped there: the larger sets below do that.)"""
    for L in W.SWEEP_L:
        case = W.sweep(L)
        sp = upload(eng, case)
        check_same(eng, sp, case, oracle_csr(case), "")
        sp.free()


@pytest.mark.parametrize("start", W.RADIX_STARTS, ids=["midnight", "7:13:37"])
@pytest.mark.parametrize("family", W.RADIX_FAMILIES)
def test_generator_forms_and_radices(eng, family, start):
    """Every second, minute and hour set size as a range, a stepped progression
    and a range with a hole, and the day-level masks: the mixed-radix digits
    and carries, the divisions by every radix, the choice of linear, affine
    and table form -- from a midnight and from 7:13:37 into a day."""
    case, _ = W.radix_case(family, start)
    sp = upload(eng, case)
    check_same(eng, sp, case, oracle_csr(case), "")
    sp.free()


def test_position_slices_whole_csr(fresh):
    """E >= 2^25: 2048-event position slices.  (a) the first call of a context
    (slice map by k_chunk_map), (b, c) a steady-state call on a poisoned larger
    buffer (slice map by the scan), (d) the same window pipelined into both
    output buffers and into one."""
    case = W.layout(W.E_POSITION)
    want = oracle_csr(case)
    sp = upload(fresh, case)
    check_same(fresh, sp, case, want, "first call")
    cap, E = steady_state(fresh, sp, case, want, "steady state")
    assert cap > E >= 1 << 25
    checksum = fresh.checksum(fresh.result_device()[1], E)
    pipelined(fresh, sp, case, cap, E, checksum, "position slices")
    sp.free()


def test_slice_mode_edge(fresh):
    """E = 2^25 - 1 (the last cost-space size), 2^25 (full position slices
    only) and 2^25 + 1 (a last slice of one event), each a steady-state call on
    a larger poisoned buffer; one oracle run, extended by the trailing one-fire
    rules in numpy."""
    base = W.layout(W.E_EDGE)
    eo, et = oracle_csr(base)
    cases = [W.extended(base, k) for k in (0, 1, 2)]
    sps = [upload(fresh, c) for c in cases]
    cap = expand(fresh, sps[2], cases[2], longer=600)
    for k in (2, 0, 1):
        want = W.extend_csr(base, eo, et, k)
        assert int(want[0][-1]) == (1 << 25) - 1 + k
        steady_state(fresh, sps[k], cases[k], want, f"E = 2^25 - 1 + {k}", cap)
    for sp in sps:
        sp.free()


@pytest.mark.parametrize("zone", ["UTC", W.LORD_HOWE])
def test_mid_cost_slices(fresh, zone):
    """E in [2^22, 2^23): cost-space slices at a shift of 8 or more, so pieces
    long enough for the writer's batch loop.  In Australia/Lord_Howe the window
    holds the 2026-04-04 transition: walked runs share blocks with closed-form
    runs (placeholders, then k_write_walk)."""
    case = W.layout(W.E_MID, zone)
    want = oracle_csr(case)
    sp = upload(fresh, case)
    check_same(fresh, sp, case, want, "first call")
    steady_state(fresh, sp, case, want, "steady state")
    sp.free()


@pytest.mark.parametrize("L", [64, 2049])
def test_short_window_guard(eng, L):
    """A short window on a buffer sized by a 24-h call of the same rules: the
    capacity is far above E, the words past E stay untouched."""
    case = W.sweep(L)
    sp = upload(eng, case)
    cap = eng.expand_device(sp, product_zone("UTC"), case.t0, case.t0 + W.DAY)
    assert cap > 5 * int(case.off[-1])
    steady_state(eng, sp, case, oracle_csr(case), "after a 24-h call", cap)
    sp.free()
