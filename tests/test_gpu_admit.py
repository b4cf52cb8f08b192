"""Admission profile on the GPU (cg_admit_*): the fires Job.limit() would admit
and those it would drop, per (rule, bucket) and per (node, bucket), against the
literal fire-by-fire model (admit_model.py) over the oracle's fire lists and
the oracle's Job.Cmds filter for the node matrix.  Exact integer equality
throughout; the first differing (row, bucket) is named.

The set: 330 rules in 88 units of 5, 2 and 1 rules, about 70 of which can drop
(more than one wave of k_admit_units, the last one partial) with units that
never drop among them (compaction); limits of 0, 1, 2 and 16 and run times
from none to past the horizon cycle over the units.  A case's model is
computed once and shared by its two kinds."""
import numpy as np
import pytest

import admit_model as AM
import inflight_model as IM
import oracle_lib as O
import profile_cases as PC
import profile_model as PM
import top_rules_model as TM
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import _lib, cron
from cronsun_amd.engine import RulesIn
from cronsun_amd.model import admission_units

pytestmark = pytest.mark.gpu

NY_SPRING = 1772953200  # 2026-03-08 07:00Z
SIZES = [5, 5, 2, 5, 1, 5, 5, 2] * 11  # 88 units, 330 rules
POOL = ["* * * * * *", "*/7 * * * * *", "@every 11s", "0 */5 * * * *", "7,30,45 * * * * *", "@every 90s",
        "0 0 0 30 Feb ?", "*/20 */2 * * * *", "0 * * * * *", "*/2 * * * * *", "30 2,32 * * * *", "@every 7s",
        "15/35 * 0-23/5 * * *", "@hourly", "58-59 * * * * *", "0 30 2 * * *", "@every 3600s", "0/15 10-12 * * * *"]
PARS = [1, 2, 1, 1, 16, 2, 1, 2, 0]


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def same(what, got, exp, row="rule"):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        at = [int(x[0]) for x in np.nonzero(got != exp)]
        where = f"{row} {at[0]} bucket {at[1]}" if got.ndim == 2 else f"bucket {at[0]}"
        raise AssertionError(f"{what}: {where}: {int(got[tuple(at)])} vs {int(exp[tuple(at)])}")


def the_specs():
    """330 specs, seeded; at most four of them fire every second (the model is
    a Python loop over the fires)."""
    rng = np.random.default_rng(330)
    specs = [POOL[i] for i in rng.integers(1, len(POOL), sum(SIZES))]
    for r in (0, 7, 12, 200):  # in units of 5, 2, 1 and 5 rules
        specs[r] = POOL[0]
    return specs


def unit_args(w):
    """(dur_ms, parallels, unit) per rule: the values cycle over the units."""
    durs = [10_000, 1001, 0, 60_000, 999, w * 1000, 25_000, 3500 * w, IM.INT64_MAX, 1000, 400_000]
    unit = np.repeat(np.arange(len(SIZES), dtype=np.int32) * 3 + 5, SIZES)  # increasing, not dense
    dur = np.repeat([durs[u % len(durs)] for u in range(len(SIZES))], SIZES).astype(np.int64)
    par = np.repeat([PARS[u % len(PARS)] for u in range(len(SIZES))], SIZES).astype(np.int64)
    return dur, par, unit


def can_drop(w, B):
    dur, par, unit = unit_args(w)
    d = np.minimum(IM.seconds(dur), w * B)
    first = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    return [not AM.never_drops(int(par[r]), int(d[r]), k) for r, k in zip(first, SIZES)]


_cases = {}


class Case:
    """One (zone, w, B): the base's fire lists, the start matrix, and the
    model's two matrices."""

    def __init__(self, zone, w, B):
        if zone == "UTC":
            t0 = PC.T0_UTC
        else:  # the horizon straddles the transition, t0 on no aligned second
            tau = NY_SPRING if zone == "America/New_York" else PC.first_transition_2026(zone)
            t0 = tau - (w * B) // 2 + 17
        specs = the_specs()
        self.zone, self.w, self.B, self.t0, self.specs = zone, w, B, t0, specs
        self.off, self.times = O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + w * B,
                                              oracle_zone(zone))
        self.dur, self.par, self.unit = unit_args(w)
        self.starts = PM.bin_fires(self.off, self.times, t0, w, B)
        self.adm, self.drop = AM.admit_from_lists(self.off, self.times, t0, w, B, self.dur, self.par, self.unit)
        assert np.array_equal(self.adm + self.drop, self.starts)


def case(zone, w, B):
    if (zone, w, B) not in _cases:
        _cases[(zone, w, B)] = Case(zone, w, B)
    return _cases[(zone, w, B)]


def upload(eng, specs):
    return eng.upload([cron.Parse(s) for s in specs])


def poison(eng):
    """0xFF over the readable profile's buffers: a cell nobody stores shows as -1."""
    r, t, n, R, N, B = eng.profile_result_device()
    eng.fill(r, R * B * 4, 0xFF)
    eng.fill(t, B * 8, 0xFF)
    if n:
        eng.fill(n, N * B * 8, 0xFF)


# ------------------------------------------------------------ rule matrix --
SHAPES = [("UTC", 3600, 1), ("UTC", 3600, 7), ("UTC", 60, 64), ("UTC", 60, 100), ("UTC", 1, 4096),
          ("America/New_York", 60, 100), ("America/New_York", 1, 4096), ("America/New_York", 3600, 7),
          ("Pacific/Chatham", 60, 100), ("Pacific/Chatham", 1, 4096), ("Pacific/Chatham", 3600, 7)]


def test_the_set_is_the_shape_the_kernel_needs():
    """More than one wave of units that can drop, a partial last wave, and
    units that never drop among them, at every shape."""
    assert sum(SIZES) == 330 and len(SIZES) == 88 and set(SIZES) == {1, 2, 5}
    for _, w, B in SHAPES:
        cd = can_drop(w, B)
        assert 64 < sum(cd) < 88 and sum(cd) % 64 != 0, (w, B, sum(cd))
        first = cd.index(False)
        assert any(cd[:first]) and any(cd[first:])  # never-drop units between droppable ones


@pytest.mark.parametrize("zone,w,B", SHAPES)
def test_rule_matrix_both_kinds(eng, zone, w, B):
    """B of 1, 7, 64, 100 and 4096 with w of 1, 60 and 3600; UTC, New York on
    its spring-forward day and Chatham across its transition.  Both kinds:
    rule matrix and totals exact, admitted + dropped == Engine.profile cell by
    cell.  The profile buffers are poisoned before each call."""
    c = case(zone, w, B)
    loc = product_zone(zone)
    sp = upload(eng, c.specs)
    starts, start_totals = eng.profile(sp, loc, c.t0, w, B)
    same("Engine.profile", starts, c.starts)
    got = {}
    for what, kind, exp in (("dropped", _lib.PROFILE_DROPPED, c.drop), ("admitted", _lib.PROFILE_ADMITTED, c.adm)):
        poison(eng)
        rules, totals = eng.admit(sp, loc, c.t0, w, B, c.dur, c.par, c.unit, what=what)
        assert eng.profile_kind() == kind
        same(f"{zone} w={w} B={B} {what} rule matrix", rules, exp)
        same(f"{what} totals", totals, exp.sum(axis=0, dtype=np.int64))
        got[what] = rules
    same("admitted + dropped", got["admitted"] + got["dropped"], starts)
    if w * B >= 4096:
        assert c.drop.any() and c.adm.any()
    # unit == None: every rule on its own
    adm1, drop1 = AM.admit_from_lists(c.off, c.times, c.t0, w, B, c.dur, c.par, None)
    poison(eng)
    same("units of one rule", eng.admit(sp, loc, c.t0, w, B, c.dur, c.par, None, what="dropped")[0], drop1)
    k_ms = eng.admit_kernel_times()
    assert len(k_ms) == 2 and k_ms[0] > 0
    sp.free()


# ---------------------------------------------------------------- per node --
def node_rules_in():
    """6 nodes, one job per unit, the rules of a unit on the same nodes: node 5
    in no list (a zero row), node 4 in every list, ExcludeNodeIDs the same
    within a unit so the exclude modes keep the membership uniform."""
    rng = np.random.default_rng(6)
    nl, el = [], []
    for u, k in enumerate(SIZES):
        nodes = sorted(set(rng.integers(0, 4, int(rng.integers(1, 4))).tolist()) | {4})
        ex = [int(rng.integers(0, 4))] if u % 3 == 0 else []
        nl += [nodes] * k
        el += [ex] * k
    R, J = sum(SIZES), len(SIZES)
    zero = np.zeros(R + 1, dtype=np.int64)
    return RulesIn(6, 0, R, J, group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.repeat(np.arange(J, dtype=np.int32), SIZES),
                   nid_off=np.cumsum([0] + [len(x) for x in nl]), nids=np.array(sum(nl, []), dtype=np.int32),
                   gid_off=zero, gids=np.zeros(0, np.int32),
                   ex_off=np.cumsum([0] + [len(x) for x in el]), ex=np.array(sum(el, []), dtype=np.int32),
                   job_pause=np.zeros(J, np.uint8))


@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
def test_node_matrix_peaks_and_top_rules(eng, mode):
    """The node matrix of both kinds equals the oracle's join applied to the
    model's rule matrix; then the peaks and each node's top rules at its peak
    bucket, on the DROPPED profile, against the numpy models."""
    c = case("UTC", 60, 100)
    rin = node_rules_in()
    utc = product_zone("UTC")
    sp, dr = upload(eng, c.specs), eng.upload_rules(rin)
    unit, split = admission_units(rin, mode)
    assert split == [] and np.array_equal(np.unique(unit, return_inverse=True)[1], np.repeat(np.arange(88), SIZES))
    for what, exp_rules in (("admitted", c.adm), ("dropped", c.drop)):
        exp, roff = PC.oracle_node_matrix(rin, mode, exp_rules)
        eng.profile_per_node(sp, utc, c.t0, c.w, c.B, dr, mode)
        poison(eng)
        got = eng.admit_per_node(sp, utc, c.t0, c.w, c.B, c.dur, c.par, unit, dr, mode, what=what)
        same(f"mode {mode} {what} node matrix", got, exp, "node")
        same("rule matrix", eng.profile_rules(), exp_rules)
        same("totals", eng.profile_totals(), exp_rules.sum(axis=0, dtype=np.int64))
        assert not got[5].any() and got[4].any()
    assert eng.profile_kind() == _lib.PROFILE_DROPPED
    peak, bucket = eng.profile_node_peaks()
    ep, eb = IM.peaks(exp)
    same("peaks", peak, ep)
    same("peak buckets", bucket, eb)
    assert (peak[5], bucket[5]) == (0, 0)
    lroff, lrules = O.node_rules(rin, mode, np.arange(6))
    TM.same("top rules at the peaks", eng.profile_top_rules(8), TM.top_rules(c.drop, lroff, lrules, eb, 8))
    b = int(eb[4])
    TM.same("cluster-wide", eng.profile_top_rules_bucket(b, 64),
            TM.top_rules(c.drop, *TM.cluster_lists(330), [b], 64))
    dr.free()
    sp.free()


# ------------------------------------------------------------ limits, state --
def code(fn, *a, **k):
    with pytest.raises(_lib.CgError) as e:
        fn(*a, **k)
    return e.value


def test_ring_limit(eng):
    """P = 17 on a saturated rule: CG_ERANGE naming it; P = 17 with d = 1 s on
    a one-rule unit never drops and is accepted (as is any P on d = 0)."""
    utc = product_zone("UTC")
    sp = upload(eng, ["@hourly", "* * * * * *", "* * * * * *"])
    e = code(eng.admit, sp, utc, PC.T0_UTC, 60, 10, [0, 5000, 60_000], [1, 1, 17], None)
    assert e.code == _lib.CG_ERANGE and "rule 2:" in e.msg
    rules, totals = eng.admit(sp, utc, PC.T0_UTC, 60, 10, [0, 5000, 1000], [1, 1, 17], None, what="admitted")
    assert rules[2].tolist() == [60] * 10 and rules[1].tolist() == [12] * 10 and rules[0].sum() == 0
    rules, _ = eng.admit(sp, utc, PC.T0_UTC, 60, 10, [0, 5000, 0], [10**9, 16, 10**12], None, what="dropped")
    assert not rules.any()  # 16 >= 5 s: never drops
    # in one unit of two every-second rules P = 17 would need d <= 8
    e = code(eng.admit, sp, utc, PC.T0_UTC, 60, 10, [0, 9000, 9000], [1, 17, 17], [0, 1, 1])
    assert e.code == _lib.CG_ERANGE and "rule 1:" in e.msg
    rules, _ = eng.admit(sp, utc, PC.T0_UTC, 60, 10, [0, 8000, 8000], [1, 17, 17], [0, 1, 1])
    assert not rules.any()
    sp.free()


def test_refusals_and_state_between_calls(eng):
    """Argument refusals name the rule and leave the previous profile readable;
    a stuck rule (Apia's skipped day) is CG_ERANGE with nothing readable; an
    admit call followed by an in-flight call leaves kind INFLIGHT; no rule is
    valid."""
    c = case("UTC", 60, 64)
    utc = product_zone("UTC")
    sp = upload(eng, c.specs)
    args = (sp, utc, c.t0, c.w, c.B)
    same("dropped", eng.admit(*args, c.dur, c.par, c.unit)[0], c.drop)

    def bad(arr, r, v):
        out = arr.copy()
        out[r] = v
        return out
    e = code(eng.admit, *args, bad(c.dur, 9, -1), c.par, c.unit)
    assert e.code == _lib.CG_EINVAL and "rule 9:" in e.msg
    e = code(eng.admit, *args, c.dur, bad(c.par, 11, -5), c.unit)
    assert e.code == _lib.CG_EINVAL and "rule 11:" in e.msg
    e = code(eng.admit, *args, c.dur, c.par, bad(c.unit, 20, 0))
    assert e.code == _lib.CG_EINVAL and "rule 20:" in e.msg and "decreases" in e.msg
    e = code(eng.admit, *args, bad(c.dur, 3, 77_000), c.par, c.unit)  # rule 3 of the unit [0, 5)
    assert e.code == _lib.CG_EINVAL and "rule 3:" in e.msg and "differ" in e.msg
    e = code(eng.admit, *args, c.dur, bad(c.par, 1, 3), c.unit)
    assert e.code == _lib.CG_EINVAL and "rule 1:" in e.msg
    L = _lib.lib()
    for what in (-1, 0, 1, 4):
        rc = L.cg_admit_device(eng._h, sp._h, eng._loc(utc).handle, c.t0, c.w, c.B, c.dur.ctypes.data,
                               c.par.ctypes.data, c.unit.ctypes.data, what)
        assert rc == _lib.CG_EINVAL
    assert L.cg_admit_device(eng._h, sp._h, eng._loc(utc).handle, c.t0, c.w, c.B, None, c.par.ctypes.data, None,
                             3) == _lib.CG_EINVAL
    with pytest.raises(ValueError):
        eng.admit(*args, c.dur, c.par, c.unit, what="inflight")
    assert eng.profile_kind() == _lib.PROFILE_DROPPED
    same("still readable", eng.profile_rules(), c.drop)

    # an in-flight call replaces it
    infl = eng.inflight(*args, c.dur)[0]
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    same("in flight after admit", infl, IM.inflight_from_lists(c.off, c.times, c.t0, c.w, c.B, IM.seconds(c.dur)))
    same("admitted after in flight", eng.admit(*args, c.dur, c.par, c.unit, what="admitted")[0], c.adm)
    assert eng.profile_kind() == _lib.PROFILE_ADMITTED

    # Apia across the skipped 2011-12-30: the message of Engine.expand, nothing readable
    scheds = [cron.Parse(s) for s in ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]]
    apia = product_zone("Pacific/Apia")
    t0 = 1325030400
    e1 = code(eng.expand, scheds, apia, t0, t0 + 5 * 86400)
    e2 = code(eng.admit, scheds, apia, t0, 3600, 120, [7_200_000] * 3, [1] * 3, None)
    assert e1.code == e2.code == _lib.CG_ERANGE and e2.msg == e1.msg and "rule 1:" in e2.msg
    for read in (eng.profile_totals, eng.profile_kind):
        with pytest.raises(_lib.CgError):
            read()
    same("after the refusal", eng.admit(*args, c.dur, c.par, c.unit)[0], c.drop)

    # no rule: valid, an empty matrix and zero totals
    rules, totals = eng.admit(sp.slice(0, 0), utc, c.t0, c.w, 24, [], [], None)
    assert rules.shape == (0, 24) and totals.shape == (24,) and not totals.any()
    assert eng.profile_kind() == _lib.PROFILE_DROPPED
    sp.free()
