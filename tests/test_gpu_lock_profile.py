"""Lock profile on the GPU (cg_lock_profile_*): the fires the KindAlone /
KindInterval lock of Cmd.Run would grant and those it would skip, per (rule,
bucket) and per (node, bucket), against the literal fire-by-fire model
(lock_model.py) over the oracle's fire lists with the oracle's lockTtl at
now = t, and the host join (join_model.py) for the node matrix.  Exact integer
equality throughout; the first differing (row, bucket) is named.

The set: test_gpu_admit.py's 330 seeded rules in 88 units of 5, 2 and 1 rules.
Kinds cycle over the units with period 11 (one COMMON among ten ALONE /
INTERVAL), AvgTime with period 9, and a non-contending first, middle or last
rule with period 7; one lock unit has no contending rule.  79 lock units are
walked: more than one wave of k_lock_units, the last one partial, with COMMON
units between them.  A case's model is computed once and shared."""
import calendar

import numpy as np
import pytest

import join_model as JM
import lock_model as LM
import oracle_lib as O
import profile_cases as PC
import profile_model as PM
import top_rules_model as TM
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import _lib, cron
from cronsun_amd.engine import RulesIn, contends_of
from cronsun_amd.model import Group, Job, JobRule, JobSet, KindAlone, KindCommon, KindInterval, lock_units
from test_gpu_admit import NY_SPRING, SIZES, the_specs

pytestmark = pytest.mark.gpu

C_, A_, I_ = LM.COMMON, LM.ALONE, LM.INTERVAL
KINDS = [A_, I_, A_, C_, I_, A_, I_, A_, I_, A_, I_]  # per unit, cycling
AVGS = [0, 999, 1000, 2500, 60_000, 3_600_000, -1500, (1 << 63) - 1, 25_000]
FIRST = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).astype(int)
NONE_CONTENDS = 4  # a one-rule INTERVAL unit whose rule reaches no lock


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


def unit_args():
    """(kind, avg_ms, unit, contends) per rule."""
    U = len(SIZES)
    unit = np.repeat(np.arange(U, dtype=np.int32) * 3 + 5, SIZES)  # increasing, not dense
    kind = np.repeat([KINDS[u % len(KINDS)] for u in range(U)], SIZES).astype(np.int32)
    avg = np.repeat([AVGS[u % len(AVGS)] for u in range(U)], SIZES).astype(np.int64)
    contends = np.ones(sum(SIZES), dtype=np.uint8)
    for u, (r0, k) in enumerate(zip(FIRST, SIZES)):
        hole = u % 7  # 1: first, 2: middle, 3: last rule of the unit; else none
        if k > 1 and hole in (1, 2, 3):
            contends[r0 + (0, k // 2, k - 1)[hole - 1]] = 0
    contends[FIRST[NONE_CONTENDS]] = 0
    return kind, avg, unit, contends


def walked_units():
    kind, _, _, contends = unit_args()
    return [bool(kind[r0] != C_ and contends[r0:r0 + k].any()) for r0, k in zip(FIRST, SIZES)]


def ttl_oracle(oscheds, zone, kind, avg, lock_ttl, log=None):
    loc = oracle_zone(zone)

    def ttl_of(r, t):
        v = O.lock_ttl(oscheds[r], t, loc, int(kind[r]), int(avg[r]), lock_ttl)
        assert v != -(1 << 63) + 1, "the reference's lockTtl never returns (OR_NO_PROGRESS)"
        if log is not None:
            log.append((r, t, v))
        return v
    return ttl_of


_cases = {}


class Case:
    """One (zone, w, B, lock_ttl): the fire lists, the start matrix and the
    model's two matrices."""

    def __init__(self, zone, w, B, lock_ttl):
        if zone == "UTC":
            t0 = PC.T0_UTC
        else:  # the horizon straddles the transition, t0 on no aligned second
            tau = NY_SPRING if zone == "America/New_York" else PC.first_transition_2026(zone)
            t0 = tau - (w * B) // 2 + 17
        specs = the_specs()
        self.zone, self.w, self.B, self.t0, self.specs, self.lock_ttl = zone, w, B, t0, specs, lock_ttl
        osch = oracle_parse_all(specs)
        self.off, self.times = O.expand_batch(O.sched_array(osch), t0, t0 + w * B, oracle_zone(zone))
        self.kind, self.avg, self.unit, self.contends = unit_args()
        self.starts = PM.bin_fires(self.off, self.times, t0, w, B)
        self.granted, self.skipped = LM.lock_from_lists(self.off, self.times, t0, w, B, self.kind, self.avg, self.unit,
                                                        self.contends,
                                                        ttl_oracle(osch, zone, self.kind, self.avg, lock_ttl))
        assert np.array_equal(self.granted + self.skipped, self.starts)


def case(zone, w, B, lock_ttl=300):
    key = (zone, w, B, lock_ttl)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


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
SHAPES = [("UTC", 3600, 1, 300), ("UTC", 60, 100, 300), ("UTC", 1, 4096, 2),
          ("America/New_York", 60, 100, 300),
          ("Pacific/Chatham", 60, 100, 600), ("Pacific/Chatham", 1, 4096, 300), ("Pacific/Chatham", 3600, 7, 300)]


def test_the_set_is_the_shape_the_kernel_needs():
    """More than 64 walked lock units and no multiple of 64 (a partial last
    wave), COMMON units between lock units (the compaction), non-contending
    rules in each position of a unit, one lock unit with none contending."""
    assert sum(SIZES) == 330 and len(SIZES) == 88 and set(SIZES) == {1, 2, 5}
    kind, avg, unit, contends = unit_args()
    wk = walked_units()
    assert sum(wk) > 64 and sum(wk) % 64 != 0, sum(wk)
    ukind = [int(kind[r0]) for r0 in FIRST]
    first_common = ukind.index(C_)
    assert any(wk[:first_common]) and any(wk[first_common:]) and ukind.count(C_) >= 8
    assert {A_, I_} <= set(ukind)
    holes = set()
    for u, (r0, k) in enumerate(zip(FIRST, SIZES)):
        if ukind[u] != C_ and k == 5:
            holes |= {i for i in range(5) if not contends[r0 + i]}
    assert {0, 2, 4} <= holes
    r0 = FIRST[NONE_CONTENDS]
    assert ukind[NONE_CONTENDS] != C_ and not contends[r0:r0 + SIZES[NONE_CONTENDS]].any() and not wk[NONE_CONTENDS]
    assert len({(int(k), int(a)) for k, a in zip(kind, avg)}) >= 25  # most (kind, AvgTime) pairs occur
    assert (np.diff(unit) >= 0).all() and len(np.unique(unit)) == 88


@pytest.mark.parametrize("zone,w,B,lock_ttl", SHAPES)
def test_rule_matrix_both_kinds(eng, zone, w, B, lock_ttl):
    """Both kinds: rule matrix and totals exact, granted + skipped ==
    Engine.profile cell by cell (so the longer zone table left the start
    profile's segments and windows alone).  The profile buffers are poisoned
    before each call."""
    c = case(zone, w, B, lock_ttl)
    loc = product_zone(zone)
    sp = upload(eng, c.specs)
    starts, _ = eng.profile(sp, loc, c.t0, w, B)
    same("Engine.profile", starts, c.starts)
    got = {}
    for what, kind, exp in (("skipped", _lib.PROFILE_LOCK_SKIPPED, c.skipped),
                            ("granted", _lib.PROFILE_LOCK_GRANTED, c.granted)):
        poison(eng)
        rules, totals = eng.lock_runs(sp, loc, c.t0, w, B, c.kind, c.avg, c.unit, c.contends, lock_ttl, what=what)
        assert eng.profile_kind() == kind
        same(f"{zone} w={w} B={B} {what} rule matrix", rules, exp)
        same(f"{what} totals", totals, exp.sum(axis=0, dtype=np.int64))
        got[what] = rules
    same("granted + skipped", got["granted"] + got["skipped"], starts)
    # the start profile after a lock call of the same horizon is unchanged
    same("Engine.profile after the lock calls", eng.profile(sp, loc, c.t0, w, B)[0], c.starts)
    assert eng.profile_kind() == _lib.PROFILE_STARTS
    if w * B >= 4096:
        assert c.skipped.any() and c.granted.any()
    k_ms = eng.lock_kernel_times()
    assert len(k_ms) == 2 and k_ms == [0, 0]  # a start profile ran last
    sp.free()


def test_every_rule_its_own_unit(eng):
    """unit == NULL and contends == NULL."""
    c = case("UTC", 60, 100)
    g1, s1 = LM.lock_from_lists(c.off, c.times, c.t0, c.w, c.B, c.kind, c.avg, None, None,
                                ttl_oracle(oracle_parse_all(c.specs), "UTC", c.kind, c.avg, 300))
    sp = upload(eng, c.specs)
    poison(eng)
    same("units of one rule, skipped", eng.lock_runs(sp, None, c.t0, c.w, c.B, c.kind, c.avg)[0], s1)
    k_ms = eng.lock_kernel_times()
    assert k_ms[0] > 0 and k_ms[1] > 0
    poison(eng)
    same("granted", eng.lock_runs(sp, None, c.t0, c.w, c.B, c.kind, c.avg, what="granted")[0], g1)
    sp.free()


# ------------------------------------------------------------ horizon end --
def _utc(*ymdhms):
    return calendar.timegm(ymdhms + (0, 0, 0))


@pytest.mark.parametrize("spec,zone,t1", [
    ("0 0 3 * * *", "UTC", _utc(2026, 1, 6, 3, 0, 20)),
    ("0 0 3 * * *", "America/New_York", NY_SPRING + 20),  # 03:00 EDT, the first second after the skipped hour
    ("0 30 2 29 Feb ?", "UTC", _utc(2028, 2, 29, 2, 30, 20)),
    ("@every 3600s", "UTC", PC.T0_UTC + 7200),  # the second fire is t1 itself
])
def test_ttl_from_fires_past_the_horizon(eng, spec, zone, t1):
    """A rule that fires in the last minute before t1: the ttl of that fire
    comes from two fires past t1 (a day, four years, two hours on).  The grant
    decisions equal the model's, and every ttl the model asked the oracle for
    equals Engine.lock_ttl_batch at now = t."""
    w, B = 60, 120
    t0 = t1 - w * B
    combos = [(k, a) for k in (A_, I_) for a in AVGS]
    # each (kind, AvgTime) as a two-rule unit: the rule, and one firing at :20 and :40 of every minute, whose
    # INTERVAL leases (38 s from :20, so :40 is skipped) end at :58 -- before the rule's own fires at :00 / :17
    specs = [spec, "20,40 * * * * *"] * len(combos)
    kind = np.repeat([k for k, _ in combos], 2).astype(np.int32)
    avg = np.repeat([a for _, a in combos], 2).astype(np.int64)
    unit = np.repeat(np.arange(len(combos), dtype=np.int32), 2)
    osch = oracle_parse_all(specs)
    off, times = O.expand_batch(O.sched_array(osch), t0, t1, oracle_zone(zone))
    last = times[off[0]:off[1]]
    assert last.size and t1 - 60 < last[-1] <= t1, "the rule must fire in the last minute"
    log = []
    g, s = LM.lock_from_lists(off, times, t0, w, B, kind, avg, unit, None,
                              ttl_oracle(osch, zone, kind, avg, 300, log))
    loc = product_zone(zone)
    sp = upload(eng, specs)
    poison(eng)
    same("granted", eng.lock_runs(sp, loc, t0, w, B, kind, avg, unit, None, 300, what="granted")[0], g)
    poison(eng)
    same("skipped", eng.lock_runs(sp, loc, t0, w, B, kind, avg, unit, None, 300, what="skipped")[0], s)
    same("granted + skipped", g + s, eng.profile(sp, loc, t0, w, B)[0])
    # the fires of the rule itself that were asked for a ttl, the last one among them for some unit
    asked = [(r, t, v) for r, t, v in log if r % 2 == 0]
    assert any(t == last[-1] for _, t, _ in asked)
    now = np.zeros(len(specs), dtype=np.int64)
    for t in sorted({t for _, t, _ in asked}):
        now[:] = t
        ttl = eng.lock_ttl_batch(sp, loc, now, kind, avg, 300)
        for r, tt, v in asked:
            if tt == t:
                assert int(ttl[r]) == v, (spec, r, t, int(ttl[r]), v)
    sp.free()


# ------------------------------------------------------------- identities --
def test_identities(eng):
    c = case("UTC", 60, 100)
    sp = upload(eng, c.specs)
    args = (sp, None, c.t0, c.w, c.B)
    R = len(c.specs)
    # all COMMON: the start profile and a zero SKIPPED
    common = np.zeros(R, dtype=np.int32)
    poison(eng)
    same("all COMMON, granted", eng.lock_runs(*args, common, c.avg, c.unit, c.contends, what="granted")[0], c.starts)
    poison(eng)
    rules, totals = eng.lock_runs(*args, common, c.avg, c.unit, c.contends, what="skipped")
    assert not rules.any() and not totals.any() and rules.shape == c.starts.shape
    # contends all zero behaves as all COMMON
    none = np.zeros(R, dtype=np.uint8)
    poison(eng)
    same("nobody contends, granted", eng.lock_runs(*args, c.kind, c.avg, c.unit, none, what="granted")[0], c.starts)
    poison(eng)
    assert not eng.lock_runs(*args, c.kind, c.avg, c.unit, none, what="skipped")[0].any()
    sp.free()
    # one-rule @every D INTERVAL units never skip: ttl = min(D - 2, lock_ttl) clamped to >= 1, below D
    every = [f"@every {d}s" for d in (1, 2, 3, 7, 60, 299, 300, 301, 302, 303, 3600, 5400)]
    sp = upload(eng, every)
    kind = np.full(len(every), I_, dtype=np.int32)
    avg = np.full(len(every), 3_600_000, dtype=np.int64)
    for lock_ttl in (2, 300, 600):
        poison(eng)
        assert not eng.lock_runs(sp, None, c.t0, 60, 100, kind, avg, None, None, lock_ttl)[0].any(), lock_ttl
    same("@every INTERVAL granted", eng.lock_runs(sp, None, c.t0, 60, 100, kind, avg, what="granted")[0],
         eng.profile(sp, None, c.t0, 60, 100)[0])
    sp.free()


# ---------------------------------------------------------------- per node --
def node_rules_in():
    """6 nodes, one job per unit.  The rules of a job differ in membership (the
    lock does not care); node 5 is in no list (a zero row), node 4 in most;
    every third job's rules carry ExcludeNodeIDs; in the five-rule jobs the
    first and the last rule share a Cmd key (the first is replaced wherever the
    last runs); rule 1 of job 0 names no node at all."""
    rng = np.random.default_rng(6)
    nl, el, keys = [], [], []
    for u, k in enumerate(SIZES):
        for i in range(k):
            nodes = sorted(set(rng.integers(0, 4, int(rng.integers(1, 4))).tolist()) | ({4} if (u + i) % 4 else set()))
            nl.append([] if (u, i) == (0, 1) else nodes)
            el.append([int(rng.integers(0, 5))] if u % 3 == 0 else [])
            keys.append(0 if (k == 5 and i == 4) else i)
    R, J = sum(SIZES), len(SIZES)
    zero = np.zeros(R + 1, dtype=np.int64)
    return RulesIn(6, 0, R, J, rule_key=np.array(keys, dtype=np.int32),
                   group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.repeat(np.arange(J, dtype=np.int32), SIZES),
                   nid_off=np.cumsum([0] + [len(x) for x in nl]), nids=np.array(sum(nl, []), dtype=np.int32),
                   gid_off=zero, gids=np.zeros(0, np.int32),
                   ex_off=np.cumsum([0] + [len(x) for x in el]), ex=np.array(sum(el, []), dtype=np.int32),
                   job_pause=np.zeros(J, np.uint8))


@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
def test_node_matrix_peaks_and_top_rules(eng, mode):
    """contends from the join's degrees; the node matrix of both kinds equals
    the host join applied to the model's rows; then the peaks and each node's
    top rules at its peak bucket, on the SKIPPED profile."""
    c = case("UTC", 60, 100)
    rin = node_rules_in()
    rn_off, _, nt_off, nt_rule = JM.join(rin, mode)
    contends = contends_of(rn_off)
    same("contends", eng.rule_contends(rin, mode), contends)
    assert not contends[1] and 0 < int((contends == 0).sum()) < 60  # the rule on no node, and replaced ones
    unit = lock_units(rin)
    osch = oracle_parse_all(c.specs)
    g, s = LM.lock_from_lists(c.off, c.times, c.t0, c.w, c.B, c.kind, c.avg, unit, contends,
                              ttl_oracle(osch, "UTC", c.kind, c.avg, 300))
    sp, dr = upload(eng, c.specs), eng.upload_rules(rin)
    for what, exp_rules in (("granted", g), ("skipped", s)):
        exp = PM.node_matrix(nt_off, nt_rule, exp_rules)
        eng.profile_per_node(sp, None, c.t0, c.w, c.B, dr, mode)
        poison(eng)
        got = eng.lock_runs_per_node(sp, None, c.t0, c.w, c.B, c.kind, c.avg, unit, contends, dr, mode, 300, what)
        same(f"mode {mode} {what} node matrix", got, exp, "node")
        same("rule matrix", eng.profile_rules(), exp_rules)
        same("totals", eng.profile_totals(), exp_rules.sum(axis=0, dtype=np.int64))
        assert not got[5].any() and got[4].any()
    assert eng.profile_kind() == _lib.PROFILE_LOCK_SKIPPED
    peak, bucket = eng.profile_node_peaks()
    ep = exp.max(axis=1)
    eb = exp.argmax(axis=1).astype(np.int32)
    same("peaks", peak, ep)
    same("peak buckets", bucket, eb)
    assert (peak[5], bucket[5]) == (0, 0)
    TM.same("top rules at the peaks", eng.profile_top_rules(8), TM.top_rules(s, nt_off, nt_rule, eb, 8))
    b = int(eb[4])
    TM.same("cluster-wide", eng.profile_top_rules_bucket(b, 64), TM.top_rules(s, *TM.cluster_lists(330), [b], 64))
    dr.free()
    sp.free()


# ------------------------------------------------------ refusals and state --
def code(fn, *a, **k):
    with pytest.raises(_lib.CgError) as e:
        fn(*a, **k)
    return e.value


def test_refusals_and_state_between_calls(eng):
    """Every CG_EINVAL leaves the previous profile and its kind readable; a
    good call reports kind 4 or 5, a start profile afterwards 0."""
    c = case("UTC", 60, 100)
    sp = upload(eng, c.specs)
    args = (sp, None, c.t0, c.w, c.B)
    same("skipped", eng.lock_runs(*args, c.kind, c.avg, c.unit, c.contends)[0], c.skipped)
    assert eng.profile_kind() == _lib.PROFILE_LOCK_SKIPPED == 5

    def bad(arr, r, v):
        out = arr.copy()
        out[r] = v
        return out
    e = code(eng.lock_runs, *args, bad(c.kind, 9, 3), c.avg, c.unit, c.contends)
    assert e.code == _lib.CG_EINVAL and "rule 9:" in e.msg and "kind" in e.msg
    e = code(eng.lock_runs, *args, bad(c.kind, 9, -1), c.avg, c.unit, c.contends)
    assert e.code == _lib.CG_EINVAL and "rule 9:" in e.msg
    e = code(eng.lock_runs, *args, c.kind, c.avg, bad(c.unit, 20, 0), c.contends)
    assert e.code == _lib.CG_EINVAL and "rule 20:" in e.msg and "decreases" in e.msg
    e = code(eng.lock_runs, *args, c.kind, bad(c.avg, 3, 77_000), c.unit, c.contends)  # rule 3 of the unit [0, 5)
    assert e.code == _lib.CG_EINVAL and "rule 3:" in e.msg and "differ" in e.msg
    e = code(eng.lock_runs, *args, bad(c.kind, 1, (int(c.kind[1]) + 1) % 3), c.avg, c.unit, c.contends)
    assert e.code == _lib.CG_EINVAL and "rule 1:" in e.msg and "differ" in e.msg
    L = _lib.lib()
    z = eng._loc(None).handle
    k, a, u, ct = c.kind.ctypes.data, c.avg.ctypes.data, c.unit.ctypes.data, c.contends.ctypes.data
    for what in (-1, 0, 1, 2, 3, 6):
        assert L.cg_lock_profile_device(eng._h, sp._h, z, c.t0, c.w, c.B, k, a, u, ct, 300, what) == _lib.CG_EINVAL
    for lock_ttl in (1, 0, -5):
        assert L.cg_lock_profile_device(eng._h, sp._h, z, c.t0, c.w, c.B, k, a, u, ct, lock_ttl, 5) == _lib.CG_EINVAL
        assert "lock_ttl" in _lib.last_error()
    assert L.cg_lock_profile_device(eng._h, sp._h, z, c.t0, c.w, c.B, None, a, u, ct, 300, 5) == _lib.CG_EINVAL
    assert L.cg_lock_profile_device(eng._h, sp._h, z, c.t0, c.w, c.B, k, None, u, ct, 300, 5) == _lib.CG_EINVAL
    assert L.cg_lock_profile_device(eng._h, sp._h, z, c.t0, c.w, 0, k, a, u, ct, 300, 5) == _lib.CG_EINVAL
    dr = eng.upload_rules(node_rules_in())
    assert L.cg_lock_profile_per_node_device(eng._h, sp._h, z, c.t0, c.w, c.B, k, a, u, ct, 300, 5, dr._h,
                                             3) == _lib.CG_EINVAL  # bad exclude mode
    assert L.cg_lock_profile_per_node_device(eng._h, sp._h, z, c.t0, c.w, c.B, k, a, u, ct, 1, 5, dr._h,
                                             0) == _lib.CG_EINVAL
    dr.free()
    with pytest.raises(ValueError):
        eng.lock_runs(*args, c.kind, c.avg, c.unit, c.contends, what="dropped")
    with pytest.raises(ValueError):
        eng.lock_runs(*args, c.kind, c.avg, c.unit, c.contends, lock_ttl=1)
    assert eng.profile_kind() == _lib.PROFILE_LOCK_SKIPPED
    same("still readable", eng.profile_rules(), c.skipped)

    same("granted", eng.lock_runs(*args, c.kind, c.avg, c.unit, c.contends, what="granted")[0], c.granted)
    assert eng.profile_kind() == _lib.PROFILE_LOCK_GRANTED == 4
    same("starts afterwards", eng.profile(*args)[0], c.starts)
    assert eng.profile_kind() == _lib.PROFILE_STARTS == 0
    # no rule: valid, an empty matrix and zero totals
    rules, totals = eng.lock_runs(sp.slice(0, 0), None, c.t0, c.w, 24, [], [])
    assert rules.shape == (0, 24) and totals.shape == (24,) and not totals.any()
    assert eng.profile_kind() == _lib.PROFILE_LOCK_SKIPPED
    sp.free()


def test_device_views(eng):
    """lock_runs_device: torch views of the engine's own buffers."""
    c = case("UTC", 60, 100)
    sp = upload(eng, c.specs)
    rules, totals = eng.lock_runs_device(sp, None, c.t0, c.w, c.B, c.kind, c.avg, c.unit, c.contends)
    same("device view", rules.cpu().numpy(), c.skipped)
    same("device totals", totals.cpu().numpy(), c.skipped.sum(axis=0, dtype=np.int64))
    sp.free()


# ----------------------------------------------------------------- job set --
def the_jobs():
    """A dozen jobs on five nodes, one group."""
    groups = {"g1": Group("g1", "g", ["n1", "n2"])}

    def job(i, kind, avg, rules, **kw):
        return Job(ID=f"job{i:02d}", Kind=kind, AvgTime=avg, Rules=[JobRule(ID=f"r{i}.{k}", Timer=t, **m)
                                                                     for k, (t, m) in enumerate(rules)], **kw)
    on = lambda *n: {"NodeIDs": list(n)}  # noqa: E731
    jobs = [
        job(0, KindAlone, 2500, [("@every 60s", on("n0", "n1", "n2"))]),  # runs every other minute
        job(1, KindAlone, 3000, [("@every 60s", on("n0", "n1"))]),  # runs every minute
        job(2, KindInterval, 0, [("0 0,1 * * * *", on("n3"))]),
        job(3, KindInterval, 10_000, [("0 * * * * *", on("n0")), ("30 * * * * *", {"GroupIDs": ["g1"]})]),
        job(4, KindCommon, 90_000, [("*/20 * * * * *", on("n0", "n3"))]),
        job(5, KindAlone, 45_000, [("*/10 * * * * *", on("n2")), ("5/10 * * * * *", on("n3", "n4"))]),
        job(6, KindInterval, 0, [("*/7 * * * * *", {"GroupIDs": ["g1"], "ExcludeNodeIDs": ["n1"]})]),
        job(7, KindAlone, 1000, [("* * * * * *", on("n4"))]),
        job(8, KindAlone, 0, [("0 */5 * * * *", on("n0")), ("0 */5 * * * *", on("n1"))]),  # a tie every five minutes
        job(9, KindInterval, 500, [("@every 90s", on("n2", "n3"))], Pause=True),  # paused: contends nowhere
        job(10, KindAlone, -200, [("15 * * * * *", {"NodeIDs": []})]),  # on no node
        job(11, KindCommon, 0, [("@hourly", on("n0", "n1", "n2", "n3", "n4"))]),
    ]
    return jobs, groups


@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE])
def test_jobset_lock_runs_and_node_skips(eng, mode):
    jobs, groups = the_jobs()
    js = JobSet(jobs, groups)
    t0, w, B = PC.T0_UTC, 60, 90
    rin = js.rules_in()
    specs = [r.Timer for r in js.rules]
    osch = oracle_parse_all(specs)
    off, times = O.expand_batch(O.sched_array(osch), t0, t0 + w * B, oracle_zone("UTC"))
    kind, avg = js.rule_kinds()
    rn_off, _, nt_off, nt_rule = JM.join(rin, mode)
    unit = np.asarray(js.rule_job, dtype=np.int32)
    same("lock_units", lock_units(rin), unit)
    g, s = LM.lock_from_lists(off, times, t0, w, B, kind, avg, unit, contends_of(rn_off),
                              ttl_oracle(osch, "UTC", kind, avg, 300))
    runs = js.job_lock_runs(t0, w, B, mode=mode, engine=eng)
    exclusive = [j.ID for j in jobs if j.Kind != KindCommon]
    assert sorted(runs) == sorted(exclusive)
    for ji, j in enumerate(jobs):
        if j.Kind == KindCommon:
            continue
        mine = unit == ji
        same(f"{j.ID} granted", runs[j.ID][0], g[mine].sum(axis=0, dtype=np.int64))
        same(f"{j.ID} skipped", runs[j.ID][1], s[mine].sum(axis=0, dtype=np.int64))
    # the 2500-ms alone job runs every other minute, the 3000-ms one every minute
    assert runs["job00"][0].tolist() == [1, 0] * 45 and runs["job00"][1].tolist() == [0, 1] * 45
    assert runs["job01"][0].tolist() == [1] * 90 and not runs["job01"][1].any()
    # a paused job and a job on no node contend nowhere: granted is their start row
    assert not runs["job09"][1].any() and not runs["job10"][1].any() and runs["job10"][0].sum() == 90
    skips = js.node_lock_skips(t0, w, B, mode=mode, engine=eng)
    exp = PM.node_matrix(nt_off, nt_rule, s)
    assert sorted(skips) == sorted(js.node_id(n) for n in range(rin.n_nodes))
    for n in range(rin.n_nodes):
        same(f"node {js.node_id(n)} skipped", skips[js.node_id(n)], exp[n])
    assert skips["n0"].any() and skips["n4"].any()
    grants = js.node_lock_skips(t0, w, B, mode=mode, engine=eng, what="granted")
    exp = PM.node_matrix(nt_off, nt_rule, g)
    for n in range(rin.n_nodes):
        same(f"node {js.node_id(n)} granted", grants[js.node_id(n)], exp[n])
