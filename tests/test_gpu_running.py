"""Running profile on the GPU (CG_PROFILE_RUNNING of cg_admit_*,
CG_PROFILE_LOCK_RUNNING of cg_lock_profile_*): commands in flight at each bucket
edge counting only the fires Job.limit() admits, or only those the job lock
grants, per (rule, bucket) and per (node, bucket), against the literal model
(running_model.py) over the oracle's fire lists -- with the oracle's lockTtl at
now = t in the lock flavour -- and the host join (join_model.py) for the node
matrix.  Exact integer equality throughout; the first differing (row, bucket)
is named.  The profile buffers are poisoned with 0xFF before each call.

The admission set is test_gpu_admit.py's: 330 seeded rules in 88 units of 5, 2
and 1 rules, more than 64 of which can drop (a partial last wave of
k_admit_units) with units that never drop among them, so k_rows_prefix skips
rows between rows it sums.  Run times cycle over the units through 0, 999,
1001, 2500, w, 3w, 3.5w, past the horizon and INT64_MAX.  The lock set is
test_gpu_lock_profile.py's, with non-contending first, middle and last rules.
B of 1 and 7 take k_rows_prefix's packed path (7: no power of two), 64 one
whole chunk, 100 a carry into a partial chunk, 4096 sixty-three carries.  A
case's model is computed once and shared."""
import numpy as np
import pytest

import admit_model as AM
import inflight_model as IM
import join_model as JM
import oracle_lib as O
import profile_cases as PC
import profile_model as PM
import running_model as RM
import test_gpu_admit as GA
import test_gpu_lock_profile as GL
import top_rules_model as TM
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import _lib
from cronsun_amd.engine import contends_of
from cronsun_amd.model import admission_units, lock_units

pytestmark = pytest.mark.gpu

SIZES, FIRST = GA.SIZES, GL.FIRST
same, poison, upload = GA.same, GA.poison, GA.upload


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def unit_args(w, B):
    """(dur_ms, parallels, unit) per rule: the values cycle over the units."""
    durs = [10_000, 1001, 0, 3 * w * 1000, 999, w * 1000, 25_000, 3500 * w, IM.INT64_MAX, 2500, (w * B + 7) * 1000]
    unit = np.repeat(np.arange(len(SIZES), dtype=np.int32) * 3 + 5, SIZES)  # increasing, not dense
    dur = np.repeat([durs[u % len(durs)] for u in range(len(SIZES))], SIZES).astype(np.int64)
    par = np.repeat([GA.PARS[u % len(GA.PARS)] for u in range(len(SIZES))], SIZES).astype(np.int64)
    return dur, par, unit


def can_drop(w, B):
    dur, par, _ = unit_args(w, B)
    d = np.minimum(IM.seconds(dur), w * B)
    return [not AM.never_drops(int(par[r]), int(d[r]), k) for r, k in zip(FIRST, SIZES)]


def t0_of(zone, w, B):
    if zone == "UTC":
        return PC.T0_UTC
    tau = GA.NY_SPRING if zone == "America/New_York" else PC.first_transition_2026(zone)
    return tau - (w * B) // 2 + 17  # the horizon straddles the transition, t0 on no aligned second


_cases = {}


class AdmitCase:
    """One (zone, w, B) of the admission flavour: fire lists and the model's
    running, admitted and in-flight matrices."""

    def __init__(self, zone, w, B):
        self.zone, self.w, self.B, self.t0, self.specs = zone, w, B, t0_of(zone, w, B), GA.the_specs()
        self.off, self.times = O.expand_batch(O.sched_array(oracle_parse_all(self.specs)), self.t0, self.t0 + w * B,
                                              oracle_zone(zone))
        self.dur, self.par, self.unit = unit_args(w, B)
        self.dsec = np.minimum(IM.seconds(self.dur), w * B)
        self.run, self.adm = RM.admit_running(self.off, self.times, self.t0, w, B, self.dur, self.par, self.unit)
        self.infl = IM.inflight_from_lists(self.off, self.times, self.t0, w, B, self.dsec)
        self.droppable = np.repeat(can_drop(w, B), SIZES)  # per rule


class LockCase:
    """One (zone, w, B, lock_ttl) of the lock flavour, on top of
    test_gpu_lock_profile's case (its fire lists and GRANTED matrix)."""

    def __init__(self, zone, w, B, lock_ttl):
        g = GL.case(zone, w, B, lock_ttl)
        self.g = g
        self.dur = np.maximum(g.avg, 0)
        self.dsec = np.minimum(IM.seconds(self.dur), w * B)
        ttl_of = GL.ttl_oracle(oracle_parse_all(g.specs), zone, g.kind, g.avg, lock_ttl)
        self.run, granted = RM.lock_running(g.off, g.times, g.t0, w, B, g.kind, g.avg, g.unit, g.contends, ttl_of)
        assert np.array_equal(granted, g.granted)
        self.infl = IM.inflight_from_lists(g.off, g.times, g.t0, w, B, self.dsec)
        self.locked = (g.kind != GL.C_) & (g.contends != 0)  # per rule: its fires go through the lock


def case(cls, *key):
    if (cls, key) not in _cases:
        _cases[(cls, key)] = cls(*key)
    return _cases[(cls, key)]


def below(what, got, cap):
    if not (got <= cap).all():
        r, b = [int(x[0]) for x in np.nonzero(got > cap)]
        raise AssertionError(f"{what}: rule {r} bucket {b}: {int(got[r, b])} > {int(cap[r, b])}")


def whole_bucket_rows(what, run, starts, dsec, w, B):
    """d == w: the start rows; d == 3w: their sliding sum over 3 buckets;
    d >= B*w: their prefix sums."""
    for m, rows in ((1, dsec == w), (3, dsec == 3 * w), (B, dsec >= w * B)):
        rows = np.nonzero(rows)[0]
        same(f"{what}: rows with d == {m} buckets", run[rows].astype(np.int64), IM.sliding_sum(starts[rows], m))
    return int((dsec == w).sum())


# ------------------------------------------------------------ rule matrix --
ADMIT_SHAPES = GA.SHAPES
LOCK_SHAPES = [("UTC", 3600, 1, 300), ("UTC", 3600, 7, 300), ("UTC", 60, 64, 300), ("UTC", 60, 100, 300),
               ("UTC", 1, 4096, 2), ("America/New_York", 60, 100, 300), ("Pacific/Chatham", 60, 100, 600),
               ("Pacific/Chatham", 1, 4096, 300), ("Pacific/Chatham", 3600, 7, 300)]


def test_the_sets_are_the_shapes_the_kernels_need():
    """More than one wave of walked units with a partial last wave and
    unwalked units among them, at every shape; every duration class occurs on
    a unit that can drop; B covers both paths of k_rows_prefix and a carry."""
    assert sum(SIZES) == 330 and len(SIZES) == 88
    for _, w, B in ADMIT_SHAPES:
        cd = can_drop(w, B)
        assert 64 < sum(cd) < 88 and sum(cd) % 64 != 0, (w, B, sum(cd))
        first = cd.index(False)
        assert any(cd[:first]) and any(cd[first:])
        dur, _, _ = unit_args(w, B)
        d = np.minimum(IM.seconds(dur), w * B)[FIRST]
        for want in (w, 3 * w, w * B):  # each whole-bucket identity has a unit that can drop
            assert want > w * B or any(c and x == want for c, x in zip(cd, d)), (w, B, want)
    assert {B for _, _, B in ADMIT_SHAPES} == {1, 7, 64, 100, 4096} == {s[2] for s in LOCK_SHAPES}
    assert {w for _, w, _ in ADMIT_SHAPES} == {1, 60, 3600} == {s[1] for s in LOCK_SHAPES}
    wk = GL.walked_units()
    assert sum(wk) > 64 and sum(wk) % 64 != 0 and not all(wk)


@pytest.mark.parametrize("zone,w,B", ADMIT_SHAPES)
def test_admission_flavour_rule_matrix(eng, zone, w, B):
    c = case(AdmitCase, zone, w, B)
    loc = product_zone(zone)
    sp = upload(eng, c.specs)
    args = (sp, loc, c.t0, w, B)
    eng.profile(*args)
    poison(eng)
    run, totals = eng.admit(*args, c.dur, c.par, c.unit, what="running")
    assert eng.profile_kind() == _lib.PROFILE_RUNNING == 7
    same(f"{zone} w={w} B={B} running rule matrix", run, c.run)
    same("running totals", totals, c.run.sum(axis=0, dtype=np.int64))
    assert eng.running_kernel_times() > 0 and eng.admit_kernel_times()[1] > 0
    # the cheap cross-checks, device against device
    poison(eng)
    infl = eng.inflight(*args, c.dur)[0]
    same("Engine.inflight", infl, c.infl)
    below("running <= in flight", run, infl)
    same("rows of units that never drop", run[~c.droppable], infl[~c.droppable])
    poison(eng)
    adm = eng.admit(*args, c.dur, c.par, c.unit, what="admitted")[0]
    assert eng.running_kernel_times() == 0
    assert whole_bucket_rows("admitted", run, adm, c.dsec, w, B) > 0
    sums = RM.unit_sums(run, c.unit)
    for u, r0 in enumerate(FIRST):
        if c.droppable[r0]:
            assert sums[u].max() <= c.par[r0], (u, int(sums[u].argmax()), int(sums[u].max()), int(c.par[r0]))
    if w * B >= 4096:
        assert (c.run < c.infl).any() and c.run.any()
    sp.free()


@pytest.mark.parametrize("zone,w,B,lock_ttl", LOCK_SHAPES)
def test_lock_flavour_rule_matrix(eng, zone, w, B, lock_ttl):
    c = case(LockCase, zone, w, B, lock_ttl)
    g = c.g
    loc = product_zone(zone)
    sp = upload(eng, g.specs)
    args = (sp, loc, g.t0, w, B)
    eng.profile(*args)
    poison(eng)
    run, totals = eng.lock_runs(*args, g.kind, g.avg, g.unit, g.contends, lock_ttl, what="running")
    assert eng.profile_kind() == _lib.PROFILE_LOCK_RUNNING == 8
    same(f"{zone} w={w} B={B} lock running rule matrix", run, c.run)
    same("lock running totals", totals, c.run.sum(axis=0, dtype=np.int64))
    assert eng.running_kernel_times() > 0 and eng.lock_kernel_times()[1] > 0
    poison(eng)
    infl = eng.inflight(*args, c.dur)[0]
    same("Engine.inflight", infl, c.infl)
    below("running <= in flight", run, infl)
    same("rows of COMMON units and of non-contending rules", run[~c.locked], infl[~c.locked])
    assert not run[g.avg <= 0].any()
    poison(eng)
    granted = eng.lock_runs(*args, g.kind, g.avg, g.unit, g.contends, lock_ttl, what="granted")[0]
    assert eng.running_kernel_times() == 0
    assert whole_bucket_rows("granted", run, granted, c.dsec, w, B) > 0
    # an ALONE unit runs one command at a time, cluster-wide
    sums = RM.unit_sums(np.where(c.locked[:, None], run, 0), g.unit)
    for u, r0 in enumerate(FIRST):
        if g.kind[r0] == GL.A_:
            assert sums[u].max() <= 1, (u, int(sums[u].argmax()), int(sums[u].max()))
    if w * B >= 4096:
        assert (c.run < c.infl).any() and c.run.any()
    sp.free()


def test_every_rule_its_own_unit(eng):
    """unit == NULL in both flavours, contends == NULL in the lock's."""
    c = case(AdmitCase, "UTC", 60, 100)
    sp = upload(eng, c.specs)
    args = (sp, None, c.t0, c.w, c.B)
    poison(eng)
    same("admission", eng.admit(*args, c.dur, c.par, None, what="running")[0],
         RM.admit_running(c.off, c.times, c.t0, c.w, c.B, c.dur, c.par, None)[0])
    g = GL.case("UTC", 60, 100)
    exp = RM.lock_running(g.off, g.times, g.t0, g.w, g.B, g.kind, g.avg, None, None,
                          GL.ttl_oracle(oracle_parse_all(g.specs), "UTC", g.kind, g.avg, 300))[0]
    poison(eng)
    same("lock", eng.lock_runs(*args, g.kind, g.avg, what="running")[0], exp)
    sp.free()


# ---------------------------------------------------------------- per node --
def peaks_and_top_rules(eng, rule_matrix, node_matrix, nt_off, nt_rule):
    peak, bucket = eng.profile_node_peaks()
    ep, eb = IM.peaks(node_matrix)
    same("peaks", peak, ep)
    same("peak buckets", bucket, eb)
    assert (peak[5], bucket[5]) == (0, 0)
    TM.same("top rules at the peaks", eng.profile_top_rules(8), TM.top_rules(rule_matrix, nt_off, nt_rule, eb, 8))
    b = int(eb[4])
    TM.same("cluster-wide", eng.profile_top_rules_bucket(b, 64),
            TM.top_rules(rule_matrix, *TM.cluster_lists(330), [b], 64))


@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
def test_admission_flavour_node_matrix_peaks_and_top_rules(eng, mode):
    c = case(AdmitCase, "UTC", 60, 100)
    rin = GA.node_rules_in()
    _, _, nt_off, nt_rule = JM.join(rin, mode)
    unit, split = admission_units(rin, mode)
    assert split == [] and np.array_equal(np.unique(unit, return_inverse=True)[1], np.repeat(np.arange(88), SIZES))
    exp = PM.node_matrix(nt_off, nt_rule, c.run)
    sp, dr = upload(eng, c.specs), eng.upload_rules(rin)
    eng.profile_per_node(sp, None, c.t0, c.w, c.B, dr, mode)
    poison(eng)
    got = eng.admit_per_node(sp, None, c.t0, c.w, c.B, c.dur, c.par, unit, dr, mode, what="running")
    assert eng.profile_kind() == _lib.PROFILE_RUNNING
    same(f"mode {mode} running node matrix", got, exp, "node")
    same("rule matrix", eng.profile_rules(), c.run)
    same("totals", eng.profile_totals(), c.run.sum(axis=0, dtype=np.int64))
    assert not got[5].any() and got[4].any()
    peaks_and_top_rules(eng, c.run, exp, nt_off, nt_rule)
    dr.free()
    sp.free()


@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
def test_lock_flavour_node_matrix_peaks_and_top_rules(eng, mode):
    """contends from the join's degrees, the job as the unit whatever its
    rules' membership."""
    g = GL.case("UTC", 60, 100)
    rin = GL.node_rules_in()
    rn_off, _, nt_off, nt_rule = JM.join(rin, mode)
    contends, unit = contends_of(rn_off), lock_units(rin)
    run = RM.lock_running(g.off, g.times, g.t0, g.w, g.B, g.kind, g.avg, unit, contends,
                          GL.ttl_oracle(oracle_parse_all(g.specs), "UTC", g.kind, g.avg, 300))[0]
    exp = PM.node_matrix(nt_off, nt_rule, run)
    sp, dr = upload(eng, g.specs), eng.upload_rules(rin)
    eng.profile_per_node(sp, None, g.t0, g.w, g.B, dr, mode)
    poison(eng)
    got = eng.lock_runs_per_node(sp, None, g.t0, g.w, g.B, g.kind, g.avg, unit, contends, dr, mode, 300, "running")
    assert eng.profile_kind() == _lib.PROFILE_LOCK_RUNNING
    same(f"mode {mode} lock running node matrix", got, exp, "node")
    same("rule matrix", eng.profile_rules(), run)
    same("totals", eng.profile_totals(), run.sum(axis=0, dtype=np.int64))
    assert not got[5].any() and got[4].any()
    peaks_and_top_rules(eng, run, exp, nt_off, nt_rule)
    dr.free()
    sp.free()


# ------------------------------------------------------ refusals and state --
def test_state_between_calls_and_refusals(eng):
    """A call of another kind before and after: the readable profile is
    replaced and profile_kind is right.  The values each entry point refused
    before are still refused and leave the profile readable."""
    c = case(AdmitCase, "UTC", 60, 64)
    g = GL.case("UTC", 60, 100)
    lc = case(LockCase, "UTC", 60, 100, 300)
    sp = upload(eng, c.specs)
    args = (sp, None, c.t0, c.w, c.B)
    same("dropped", eng.admit(*args, c.dur, c.par, c.unit, what="dropped")[0],
         PM.bin_fires(c.off, c.times, c.t0, c.w, c.B) - c.adm)
    assert eng.profile_kind() == _lib.PROFILE_DROPPED
    same("running after dropped", eng.admit(*args, c.dur, c.par, c.unit, what="running")[0], c.run)
    assert eng.profile_kind() == _lib.PROFILE_RUNNING
    L = _lib.lib()
    z = eng._loc(None).handle
    for what in (-1, 0, 1, 4, 6, 8):
        assert L.cg_admit_device(eng._h, sp._h, z, c.t0, c.w, c.B, c.dur.ctypes.data, c.par.ctypes.data,
                                 c.unit.ctypes.data, what) == _lib.CG_EINVAL, what
    with pytest.raises(ValueError):
        eng.admit(*args, c.dur, c.par, c.unit, what="inflight")
    assert eng.profile_kind() == _lib.PROFILE_RUNNING
    same("still readable", eng.profile_rules(), c.run)
    same("in flight after running", eng.inflight(*args, c.dur)[0], c.infl)
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT and eng.running_kernel_times() == 0

    largs = (sp, None, g.t0, g.w, g.B)
    same("lock running after in flight",
         eng.lock_runs(*largs, g.kind, g.avg, g.unit, g.contends, 300, what="running")[0], lc.run)
    assert eng.profile_kind() == _lib.PROFILE_LOCK_RUNNING
    k, a, u, ct = g.kind.ctypes.data, g.avg.ctypes.data, g.unit.ctypes.data, g.contends.ctypes.data
    for what in (-1, 0, 1, 2, 3, 6, 7):
        assert L.cg_lock_profile_device(eng._h, sp._h, z, g.t0, g.w, g.B, k, a, u, ct, 300, what) == _lib.CG_EINVAL, what
    with pytest.raises(ValueError):
        eng.lock_runs(*largs, g.kind, g.avg, g.unit, g.contends, 300, what="dropped")
    assert eng.profile_kind() == _lib.PROFILE_LOCK_RUNNING
    same("still readable", eng.profile_rules(), lc.run)
    same("skipped after lock running", eng.lock_runs(*largs, g.kind, g.avg, g.unit, g.contends, 300)[0], g.skipped)
    assert eng.profile_kind() == _lib.PROFILE_LOCK_SKIPPED
    same("running after skipped", eng.admit(*args, c.dur, c.par, c.unit, what="running")[0], c.run)
    same("starts after running", eng.profile(*args)[0], PM.bin_fires(c.off, c.times, c.t0, c.w, c.B))
    assert eng.profile_kind() == _lib.PROFILE_STARTS

    # no rule: valid, an empty matrix and zero totals
    rules, totals = eng.admit(sp.slice(0, 0), None, c.t0, c.w, 24, [], [], None, what="running")
    assert rules.shape == (0, 24) and not totals.any() and eng.profile_kind() == _lib.PROFILE_RUNNING
    sp.free()


# ------------------------------------------- the unit walks' shared uploads --
def _shared_upload_sets():
    """Two rule sets off the builders above.  Small: the first 37 rules in their
    units (a single partial wave of units).  Large: the first 300 rules, every
    rule its own unit (more than one block of units, the last one partial)."""
    specs, (kind, avg, lunit, contends) = GA.the_specs(), GL.unit_args()
    sets = {}
    for name, R, grouped in (("small", 37, True), ("large", 300, False)):
        sets[name] = dict(specs=specs[:R], grouped=grouped, kind=kind[:R].copy(), avg=avg[:R].copy(),
                          lunit=lunit[:R].copy() if grouped else None, contends=contends[:R].copy())
    return sets


def _unit_counts(s, w, B):
    """(units that can drop, lock units with a contending rule) of a set."""
    R = len(s["specs"])
    dur, par, unit = (x[:R] for x in unit_args(w, B))
    ids = unit if s["grouped"] else np.arange(R)
    d = np.minimum(IM.seconds(dur), w * B)
    drop = lock = 0
    for u in np.unique(ids):
        rows = np.nonzero(ids == u)[0]
        drop += not AM.never_drops(int(par[rows[0]]), int(d[rows[0]]), len(rows))
        lock += bool(s["kind"][rows[0]] != GL.C_ and s["contends"][rows].any())
    return drop, lock


def _shared_upload_call(eng, s, what, w, B):
    """One call on set s, its arrays copied to the host: a tuple of arrays."""
    R = len(s["specs"])
    sp = upload(eng, s["specs"])
    dur, par, unit = (x[:R].copy() for x in unit_args(w, B))
    if not s["grouped"]:
        unit = None
    t0 = PC.T0_UTC
    if what.startswith("admit"):
        out = eng.admit(sp, None, t0, w, B, dur, par, unit, what=what[6:])
    elif what.startswith("lock"):
        out = eng.lock_runs(sp, None, t0, w, B, s["kind"], s["avg"], s["lunit"], s["contends"], 300, what=what[5:])
    else:
        out = eng.expand_verdicts(sp, None, t0, t0 + 3600, (dur, par, unit),
                                  (s["kind"], s["avg"], s["lunit"], s["contends"], 300))
    sp.free()
    return tuple(np.array(x) for x in out)


def test_unit_uploads_shared_between_kinds_and_sets():
    """The profile and the verdict calls upload their units, flags and error
    words into one set of buffers: on one engine, calls of every kind
    interleaved over a small and a large rule set -- so the buffers grow and
    are then reused by another kind with fewer units -- each give what the same
    call gives as the first call of a fresh engine.  One hour in UTC; B = 5 and
    B = 70, either side of the 64-lane tile switch and no power of two."""
    from cronsun_amd.engine import Engine
    sets = _shared_upload_sets()
    shapes = {5: 720, 70: 51}  # B: w, at most one hour
    for B, w in shapes.items():
        drop, lock = _unit_counts(sets["small"], w, B)
        assert 0 < drop < 64 and 0 < lock < 64, (B, drop, lock)
        drop, lock = _unit_counts(sets["large"], w, B)
        assert drop > 64 and drop % 64 and lock > 64 and lock % 64, (B, drop, lock)
    calls = [("small", "admit.dropped", 5), ("large", "lock.skipped", 70), ("small", "verdicts", 70),
             ("large", "admit.running", 70), ("small", "lock.running", 5), ("large", "verdicts", 5),
             ("small", "admit.running", 70), ("large", "admit.dropped", 5), ("small", "lock.skipped", 70),
             ("large", "lock.running", 5), ("small", "verdicts", 5)]
    exp = []
    for name, what, B in calls:
        fresh = Engine(0)
        exp.append(_shared_upload_call(fresh, sets[name], what, shapes[B], B))
        fresh.close()
    one = Engine(0)
    for (name, what, B), e in zip(calls, exp):
        got = _shared_upload_call(one, sets[name], what, shapes[B], B)
        assert len(got) == len(e)
        for i, (g, x) in enumerate(zip(got, e)):
            assert g.dtype == x.dtype and np.array_equal(g, x), (name, what, B, i)
        assert any(x.any() for x in e[-1:]), (name, what, B)  # the kind's own output is not all zero
    one.close()
