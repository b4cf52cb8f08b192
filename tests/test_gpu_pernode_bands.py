"""Per-node lists across rule bands: the whole per-node CSR at K > 1 against
the host model of tests/bands_cases.py (the oracle's fires of the distinct
kinds, assembled in numpy; tests/test_bands_cases.py holds it to the oracle
with no shortcut).  Every node, every event, bit-exact: node offsets, int64
times, int32 rules.  Every test asserts the band shape it ran with through
cg_node_result_bands: since bands hold at least 32768 rules, a per-node test
of fewer rules runs with one band whatever it was written for.

  edges3       K = 3: rules placed at the band boundaries, empty segments
  many_nodes3  K = 3, N * K > 131 072 segments (k_seg_records: per > 1)
  overflow3    K = 3, 3 days: record positions past 32 bits
  xcd35        K = 35 past 2^20 rules: band groups, time-order tile cuts
  xcd35_many   K = 35, N * K > 131 072: band groups with per > 1

Left out: the rule-ordered writer's switch to band-major tasks at K >= 128
needs more than 4.1 M rules at this band floor; the band-major task order
itself runs here through the time-order writer.
"""
import contextlib

import numpy as np
import pytest

import bands_cases as BC
from common import product_zone
from cronsun_amd import _lib

pytestmark = pytest.mark.gpu
B = BC.B


@contextlib.contextmanager
def loaded(case, order=_lib.NODE_ORDER_RULE):
    """a fresh engine with the case's schedules and rules uploaded"""
    from cronsun_amd.engine import Engine
    eng = Engine(0)
    sp = dr = None
    try:
        arr = BC.schedules(case)
        sp = eng.upload_c(arr, BC.n_rules(case))
        dr = eng.upload_rules(BC.rules_in(case))
        eng.set_node_order(order)
        yield eng, sp, dr
    finally:
        for h in (dr, sp):
            if h is not None:
                h.free()
        eng.close()


def run(eng, sp, dr, case, t0, t1):
    E, nnz = eng.expand_per_node_rules_device(sp, product_zone(case.zone), t0, t1, dr, _lib.EXCLUDE_NONE)
    assert nnz == len(case.nids)
    return eng.node_result(case.n_nodes, E)


def assert_csr(got, exp, what):
    """bit-exact, with the first difference named by node, position and band"""
    off, time, rule = got
    e_off, e_time, e_rule = exp
    assert off.dtype == np.int64 and time.dtype == np.int64 and rule.dtype == np.int32
    if not np.array_equal(off, e_off):
        n = int(np.flatnonzero(off != e_off)[0])
        pytest.fail(f"{what}: node_off[{n}] = {off[n]}, expected {e_off[n]}")
    assert len(time) == len(rule) == len(e_time)
    for col, g, e in (("time", time, e_time), ("rule", rule, e_rule)):
        bad = np.flatnonzero(g != e)
        if len(bad):
            i = int(bad[0])
            n = int(np.searchsorted(e_off, i, side="right")) - 1
            pytest.fail(f"{what}: {len(bad)} {col}s differ, the first at event {i} = node {n} + {i - e_off[n]} "
                        f"(expected rule {e_rule[i]}, band {e_rule[i] // B}): got {g[i]}, expected {e[i]}")


@pytest.mark.parametrize("name", list(BC.CASES))
def test_rule_order_whole_result(name):
    """Rule order on a fresh engine (the first call grows the output and
    relaunches the writer with its tickets reset), then again on the cached
    join and segment bounds."""
    case = BC.CASES[name]()
    exp = BC.expected(case)
    with loaded(case) as (eng, sp, dr):
        with pytest.raises(_lib.CgError) as err:
            eng.node_bands()
        assert err.value.code == _lib.CG_EINVAL
        for call in ("first", "cached"):
            got = run(eng, sp, dr, case, case.t0, case.t1)
            assert eng.node_bands() == (B, case.K)
            assert_csr(got, exp, f"{name} {call}")


@pytest.mark.parametrize("name", ["edges3", "many_nodes3", "xcd35", "xcd35_many"])
def test_time_order_direct_whole_result(name):
    """cg_set_node_order(TIME): the packed writer in band-major task order and
    the tile sort (past 2^20 rules its tiles are cut at band offsets)."""
    case = BC.CASES[name]()
    exp = BC.expected_by_time(case)
    with loaded(case, _lib.NODE_ORDER_TIME) as (eng, sp, dr):
        got = run(eng, sp, dr, case, case.t0, case.t1)
        assert eng.node_bands() == (B, case.K)
        assert eng.node_order_by_time() == 0.0  # already ordered
        assert_csr(got, exp, name)


@pytest.mark.parametrize("name", ["edges3", "xcd35"])
def test_time_order_pass_whole_result(name):
    """rule order, then cg_node_result_order_by_time"""
    case = BC.CASES[name]()
    exp = BC.expected_by_time(case)
    with loaded(case) as (eng, sp, dr):
        got = run(eng, sp, dr, case, case.t0, case.t1)
        assert eng.node_bands() == (B, case.K)
        eng.node_order_by_time()
        assert_csr(eng.node_result(case.n_nodes, len(got[1])), exp, name)


def test_band_width_changes_under_cached_join():
    """One engine, one uploaded rule set: 600 s (3 bands), a window short
    enough for wider bands, 600 s again.  The cached segment bounds are keyed
    by the band shape; every result is whole and exact."""
    case = BC.edges3()
    shapes = []
    with loaded(case) as (eng, sp, dr):
        for t1 in (case.t1, case.t0 + BC.EDGES3_SHORT, case.t1):
            got = run(eng, sp, dr, case, case.t0, t1)
            shapes.append(eng.node_bands())
            assert_csr(got, BC.expected(case, case.t0, t1), f"edges3 to +{t1 - case.t0} s {shapes[-1]}")
    assert shapes[0] == shapes[2] == (B, 3)
    assert shapes[1][0] > B and shapes[1][1] < 3, shapes


@pytest.mark.parametrize("order", ["rule", "time"])
@pytest.mark.parametrize("name,secs", [("edges3", 300), ("xcd35", 60)])
def test_pipelined_windows_whole_result(name, secs, order):
    """One synchronous call on the case's own (longer) window sizes the
    outputs and fixes the bands; then four consecutive pipelined windows on
    those bands.  The last window's whole CSR and the all-window total against
    the model."""
    case = BC.CASES[name]()
    timed = order == "time"
    wins = [(case.t0 + i * secs, case.t0 + (i + 1) * secs) for i in range(4)]
    assert secs < case.t1 - case.t0
    exp = BC.expected_by_time(case, *wins[-1]) if timed else BC.expected(case, *wins[-1])
    with loaded(case, _lib.NODE_ORDER_TIME if timed else _lib.NODE_ORDER_RULE) as (eng, sp, dr):
        run(eng, sp, dr, case, case.t0, case.t1)
        assert eng.node_bands() == (B, case.K)
        for a, b in wins:
            eng.expand_per_node_async(sp, product_zone(case.zone), a, b, dr, _lib.EXCLUDE_NONE)
        En, total = eng.expand_per_node_wait(with_total=True)
        assert eng.node_bands() == (B, case.K)
        got = eng.node_result(case.n_nodes, En)
    assert total == sum(BC.total_events(case, a, b) for a, b in wins)
    assert_csr(got, exp, f"{name} {order} window 4")
