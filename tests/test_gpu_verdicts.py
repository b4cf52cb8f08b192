"""Fire verdicts on the GPU (cg_expand_verdicts_device, cg_verdicts_*): one byte
per fire of the rule-major expansion -- bit 0: Job.limit() would drop it, bit 1:
the KindAlone / KindInterval lock would skip it -- and the selection of the
fires with given bits, against the literal fire-by-fire model
(verdict_model.py) over the oracle's fire lists with the oracle's lockTtl at
now = t.  Exact integer equality throughout; the first differing (rule, fire
index) is named.

The set: test_gpu_admit.py's 330 seeded rules in 88 units of 5, 2 and 1 rules
with its admission arguments and test_gpu_lock_profile.py's lock arguments:
more than one wave of walked units in both walks, a partial last wave, and
never-drop / COMMON units between them.  A case's oracle lists and model bytes
are computed once and shared.  The verdict bytes and the selection are
poisoned with 0xFF between two identical calls, so a byte nobody stores shows
as 255."""
import calendar

import numpy as np
import pytest

import oracle_lib as O
import profile_cases as PC
import verdict_model as VM
from common import oracle_parse_all, oracle_zone, product_zone
from cronsun_amd import _lib, cron
from cronsun_amd.model import Group, Job, JobRule, JobSet, KindAlone, KindCommon, KindInterval, admission_units
from test_gpu_admit import NY_SPRING, SIZES, the_specs, unit_args
from test_gpu_lock_profile import ttl_oracle
from test_gpu_lock_profile import unit_args as lock_unit_args

pytestmark = pytest.mark.gpu

D, S = _lib.VERDICT_DROPPED, _lib.VERDICT_SKIPPED
W_ARGS = 60  # the w test_gpu_admit.unit_args scales two of its durations by


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def upload(eng, specs):
    return eng.upload([cron.Parse(s) for s in specs])


def same(what, off, got, exp):
    d = VM.first_diff(off, got, exp)
    assert d is None, f"{what}: {d}"
    assert got.dtype == exp.dtype, (what, got.dtype, exp.dtype)


def lock_tuple(lock_ttl=300):
    kind, avg, unit, contends = lock_unit_args()
    return kind, avg, unit, contends, lock_ttl


_cases = {}


class Case:
    """One (zone, horizon): the oracle's lists and the model's bytes for
    admission, lock with LockTtl 300 and lock with LockTtl 2."""

    def __init__(self, zone, H):
        if zone == "UTC":
            t0 = PC.T0_UTC
        else:  # the horizon straddles the transition, t0 on no aligned second
            tau = NY_SPRING if zone == "America/New_York" else PC.first_transition_2026(zone)
            t0 = tau - H // 2 + 17
        self.zone, self.t0, self.t1, self.specs = zone, t0, t0 + H, the_specs()
        self.osch = oracle_parse_all(self.specs)
        self.off, self.times = O.expand_batch(O.sched_array(self.osch), t0, t0 + H, oracle_zone(zone))
        self.admit = unit_args(W_ARGS)
        self._bytes = {}

    def bytes(self, mode):
        """mode: 'admit', 'lock300', 'lock2' or 'both' (admit | lock300: the bits are independent)."""
        if mode == "both":
            return self.bytes("admit") | self.bytes("lock300")
        if mode not in self._bytes:
            if mode == "admit":
                v = VM.verdicts_from_lists(self.off, self.times, self.t0, self.t1, admit=self.admit)
            else:
                ttl = int(mode[4:])
                kind, avg, unit, contends = lock_unit_args()
                v = VM.verdicts_from_lists(self.off, self.times, self.t0, self.t1, lock=(kind, avg, unit, contends),
                                           ttl_of=ttl_oracle(self.osch, self.zone, kind, avg, ttl))
            self._bytes[mode] = v
        return self._bytes[mode]

    def args(self, mode):
        return {"admit": (self.admit, None), "lock300": (None, lock_tuple(300)), "lock2": (None, lock_tuple(2)),
                "both": (self.admit, lock_tuple(300))}[mode]


def case(zone, H):
    if (zone, H) not in _cases:
        _cases[(zone, H)] = Case(zone, H)
    return _cases[(zone, H)]


def poisoned_call(eng, sp, loc, t0, t1, admit, lock):
    """The call, 0xFF over its bytes, the same call again: (offsets, times,
    verdict) of the second, which must have stored every byte."""
    n = eng.expand_verdicts_device(sp, loc, t0, t1, admit, lock)
    p, n1 = eng.verdicts_device()
    assert n1 == n
    if n:
        eng.fill(p, n, 0xFF)
    off, times, v = eng.expand_verdicts(sp, loc, t0, t1, admit, lock)
    assert len(times) == len(v) == n
    return off, times, v


# ------------------------------------------------------ bytes vs the model --
HORIZONS = [("UTC", 1), ("UTC", 7), ("UTC", 4096), ("UTC", 25_200), ("America/New_York", 6000),
            ("America/New_York", 25_200), ("Pacific/Chatham", 6000)]


@pytest.mark.parametrize("mode", ["admit", "lock300", "lock2", "both"])
@pytest.mark.parametrize("zone,H", HORIZONS)
def test_bytes_against_the_model(eng, zone, H, mode):
    """Admission only, lock only (LockTtl 300 and 2) and both, on horizons of
    1 s to 7 h: UTC reaches the rank path only, New York and Chatham across
    their transitions the walked-run search.  offsets and times equal the
    oracle's and a plain expand_device of the same arguments."""
    c = case(zone, H)
    loc = product_zone(zone)
    sp = upload(eng, c.specs)
    admit, lock = c.args(mode)
    off, times, v = poisoned_call(eng, sp, loc, c.t0, c.t1, admit, lock)
    assert np.array_equal(off, c.off), "offsets differ from the oracle's"
    same(f"{zone} {H} s times vs the oracle", c.off, times, c.times)
    same(f"{zone} {H} s {mode} verdicts", c.off, v, c.bytes(mode))
    # the verdict call's result is the readable expansion result, and a plain call's
    n = eng.result_device()[2]
    assert n == len(times)
    off2, times2 = eng.expand(sp, loc, c.t0, c.t1)
    assert np.array_equal(off2, off)
    same("times vs Engine.expand", c.off, times, times2)
    if H >= 4096:
        exp = c.bytes(mode)
        assert exp.any() and (exp == 0).any()
        if mode == "both":
            assert (exp == (D | S)).any()
    sp.free()


def test_the_set_reaches_both_paths():
    """The walked-run search is reached in the zones with a transition: some
    fire of a walked unit lies in the hour around it."""
    for zone in ("America/New_York", "Pacific/Chatham"):
        c = case(zone, 6000)
        tau = NY_SPRING if zone == "America/New_York" else PC.first_transition_2026(zone)
        near = (c.times > tau - 1800) & (c.times <= tau + 1800)
        assert (c.bytes("admit")[near] != 0).any() and (c.bytes("lock300")[near] != 0).any()


# ------------------------------------------------- several plan segments --
def test_several_plan_segments(eng):
    """40 sparse rules over 70 days in New York from 2026-02-01T00:00:17Z (the
    spring-forward inside): run offsets of many segments per rule."""
    base = ["@hourly", "@daily", "@every 3600s", "0 30 2 * * *", "0 0 0 30 Feb ?", "0 0 0 29 Feb ?", "0 0 */6 * * *",
            "0 15 3 * * Sun"]
    specs = [base[i % len(base)] for i in range(40)]
    t0 = calendar.timegm((2026, 2, 1, 0, 0, 17))
    t1 = t0 + 70 * 86400
    zone = "America/New_York"
    osch = oracle_parse_all(specs)
    off, times = O.expand_batch(O.sched_array(osch), t0, t1, oracle_zone(zone))
    assert off[5] == off[4] and off[6] == off[5] and off[4] > off[3]  # rules 4 and 5 never fire here
    sizes = [1, 2, 2, 1, 2] * 5
    unit = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    dur = np.repeat([(5_400_000, 3 * 86_400_000)[u % 2] for u in range(len(sizes))], sizes).astype(np.int64)
    par = np.repeat([(1, 2, 1)[u % 3] for u in range(len(sizes))], sizes).astype(np.int64)
    kind = np.repeat([(1, 2, 0, 1)[u % 4] for u in range(len(sizes))], sizes).astype(np.int32)
    avg = dur.copy()
    exp = VM.verdicts_from_lists(off, times, t0, t1, admit=(dur, par, unit), lock=(kind, avg, unit, None),
                                 ttl_of=ttl_oracle(osch, zone, kind, avg, 300))
    assert (exp & D).any() and (exp & S).any() and (exp == 0).any()
    sp = upload(eng, specs)
    goff, gtimes, v = poisoned_call(eng, sp, product_zone(zone), t0, t1, (dur, par, unit),
                                    (kind, avg, unit, None, 300))
    assert np.array_equal(goff, off)
    same("times", off, gtimes, times)
    same("70 days, both passes", off, v, exp)
    sp.free()


# -------------------------------------------------------------------- edges --
def test_edges(eng):
    utc = product_zone("UTC")
    t0 = PC.T0_UTC
    # R = 0
    sp = upload(eng, ["@hourly"])
    off, times, v = eng.expand_verdicts(sp.slice(0, 0), utc, t0, t0 + 60, admit=([], [], None))
    assert off.tolist() == [0] and len(times) == 0 and len(v) == 0
    so, st = eng.verdicts_select(3, 0)
    assert so.tolist() == [0] and len(st) == 0
    sp.free()
    # only never-fire rules: E = 0
    sp = upload(eng, ["0 0 0 30 Feb ?"] * 3)
    off, times, v = eng.expand_verdicts(sp, utc, t0, t0 + 3600, admit=([5000] * 3, [1] * 3, [0, 0, 1]),
                                        lock=([1, 1, 2], [0, 0, 0], [0, 0, 1], None, 300))
    assert off.tolist() == [0, 0, 0, 0] and len(v) == 0
    so, st = eng.verdicts_select(1, 1)
    assert so.tolist() == [0, 0, 0, 0] and len(st) == 0
    sp.free()
    # no unit can drop and every unit is COMMON: no walk, all bytes 0 and all written
    specs = ["* * * * * *", "*/7 * * * * *", "@every 11s"]
    sp = upload(eng, specs)
    off, times, v = poisoned_call(eng, sp, utc, t0, t0 + 4099, ([0, 9000, 10**6], [1, 16, 0], None),
                                  ([0, 0, 0], [5000] * 3, None, None, 300))
    assert len(v) == off[3] > 4099 and off[1] == 4099 and not v.any()
    sp.free()
    # a flagged rule with zero fires between two flagged rules with fires
    specs = ["*/10 * * * * *", "0 0 0 30 Feb ?", "*/15 * * * * *"]
    osch = oracle_parse_all(specs)
    eo, et = O.expand_batch(O.sched_array(osch), t0, t0 + 5000, oracle_zone("UTC"))
    admit = ([25_000] * 3, [1] * 3, [4, 4, 4])
    lock = ([2] * 3, [0] * 3, [4, 4, 4], None, 300)
    exp = VM.verdicts_from_lists(eo, et, t0, t0 + 5000, admit=admit, lock=lock[:4],
                                 ttl_of=ttl_oracle(osch, "UTC", lock[0], lock[1], 300))
    sp = upload(eng, specs)
    off, times, v = poisoned_call(eng, sp, utc, t0, t0 + 5000, admit, lock)
    assert np.array_equal(off, eo) and eo[1] == eo[2] and (exp & D).any() and (exp & S).any()
    same("an empty flagged rule between two", eo, v, exp)
    sp.free()


def test_first_and_last_rule_are_walked():
    """Rule 0 and rule 329 belong to units that can drop and to walked lock
    units (the first and the last lane of both walks' compacted lists): the
    model drops fires of both rules and skips fires of the first unit (the
    last lock unit's one contending rule does not fire in this horizon: its
    lane walks an empty unit)."""
    from test_gpu_admit import can_drop
    from test_gpu_lock_profile import walked_units
    cd, wk = can_drop(W_ARGS, 4096 // W_ARGS), walked_units()
    assert cd[0] and cd[-1] and wk[0] and wk[-1]
    c = case("UTC", 4096)
    v = c.bytes("admit")
    assert v[c.off[0]:c.off[1]].any() and v[c.off[329]:c.off[330]].any()
    v = c.bytes("lock300")
    assert v[c.off[0]:c.off[5]].any()


# --------------------------------------------------------------- identities --
def binned(off, times, keep, t0, w, B):
    R = len(off) - 1
    rule = np.repeat(np.arange(R), np.diff(off))
    out = np.zeros((R, B), dtype=np.int32)
    np.add.at(out, (rule[keep], ((times[keep] - t0 - 1) // w)), 1)
    return out


def same_matrix(what, got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        r, b = [int(x[0]) for x in np.nonzero(got != exp)]
        raise AssertionError(f"{what}: rule {r} bucket {b}: {int(got[r, b])} vs {int(exp[r, b])}")


@pytest.mark.parametrize("zone", ["UTC", "America/New_York"])
@pytest.mark.parametrize("w,B", [(60, 100), (1, 4096), (3600, 7)])
def test_identities_with_the_profiles(eng, zone, w, B):
    """With t1 = t0 + w * B the fires with bit 0, binned, are Engine.admit's
    DROPPED matrix and those without it the ADMITTED one; bit 1 against
    Engine.lock_runs' SKIPPED / GRANTED."""
    t0 = PC.T0_UTC if zone == "UTC" else NY_SPRING - (w * B) // 2 + 17
    loc = product_zone(zone)
    specs = the_specs()
    sp = upload(eng, specs)
    admit, lock = unit_args(W_ARGS), lock_tuple(300)
    off, times, v = eng.expand_verdicts(sp, loc, t0, t0 + w * B, admit, lock)
    for what, keep in (("dropped", (v & D) != 0), ("admitted", (v & D) == 0)):
        same_matrix(f"{zone} w={w} B={B} bit 0 vs admit({what})", binned(off, times, keep, t0, w, B),
                    eng.admit(sp, loc, t0, w, B, *admit, what=what)[0])
    for what, keep in (("skipped", (v & S) != 0), ("granted", (v & S) == 0)):
        same_matrix(f"{zone} w={w} B={B} bit 1 vs lock_runs({what})", binned(off, times, keep, t0, w, B),
                    eng.lock_runs(sp, loc, t0, w, B, *lock[:4], lock_ttl=300, what=what)[0])
    sp.free()


# ---------------------------------------------------------------- selection --
def test_selection(eng):
    c = case("America/New_York", 6000)
    loc = product_zone(c.zone)
    sp = upload(eng, c.specs)
    exp = c.bytes("both")
    eng.expand_verdicts_device(sp, loc, c.t0, c.t1, *c.args("both"))
    for mask, value in ((1, 1), (2, 2), (3, 0), (3, 3), (3, 1), (3, 2)):
        eo, et = VM.select(c.off, c.times, exp, mask, value)
        n = eng.verdicts_select_device(mask, value)
        assert n == len(et), (mask, value, n, len(et))
        po, pt, n1 = eng.verdicts_selected_device()  # poison, select again: every word is stored
        assert n1 == n
        eng.fill(po, (len(c.off)) * 8, 0xFF)
        if n:
            eng.fill(pt, n * 8, 0xFF)
        so, st = eng.verdicts_select(mask, value)
        assert np.array_equal(so, eo), f"({mask}, {value}) sel_off: rule {int(np.nonzero(so != eo)[0][0])}"
        same(f"({mask}, {value}) sel_times", eo, st, et)
        assert len(et) > 0
    ms = eng.verdict_times()
    assert len(ms) == 6 and ms[0] > 0 and ms[1] > 0 and ms[4] > 0 and ms[5] > 0
    for bad in ((0, 0), (4, 0), (1, 2), (2, 1), (3, 4), (-1, 0)):
        with pytest.raises(_lib.CgError) as e:
            eng.verdicts_select(*bad)
        assert e.value.code == _lib.CG_EINVAL
    # an admission-only call: no fire has bit 1 (empty), every fire has it clear (everything)
    eng.expand_verdicts_device(sp, loc, c.t0, c.t1, *c.args("admit"))
    so, st = eng.verdicts_select(2, 2)
    assert len(st) == 0 and not so.any()
    so, st = eng.verdicts_select(2, 0)
    assert np.array_equal(so, c.off)
    same("everything", c.off, st, c.times)
    sp.free()


# -------------------------------------------------------------------- state --
def code(fn, *a, **k):
    with pytest.raises(_lib.CgError) as e:
        fn(*a, **k)
    return e.value


def test_state_and_refusals(eng):
    c = case("UTC", 4096)
    utc = product_zone("UTC")
    sp = upload(eng, c.specs)
    admit, lock = c.args("both")
    # a profile made before the verdict call reads back unchanged after it
    rules0, totals0 = eng.admit(sp, utc, c.t0, 64, 64, *admit, what="dropped")
    kind0 = eng.profile_kind()
    a = eng.expand_verdicts(sp, utc, c.t0, c.t1, admit, lock)[2]
    b = eng.expand_verdicts(sp, utc, c.t0, c.t1, admit, lock)[2]
    same("two identical calls", c.off, a, b)
    same("both", c.off, a, c.bytes("both"))
    assert eng.profile_kind() == kind0
    assert np.array_equal(eng.profile_rules(), rules0) and np.array_equal(eng.profile_totals(), totals0)

    # argument errors: the profile calls' codes, naming the same rule; all before any device work
    def bad(arr, r, x):
        out = np.array(arr).copy()
        out[r] = x
        return out
    dur, par, unit = admit
    kind, avg, lunit, contends, ttl = lock
    args = (sp, utc, c.t0, c.t1)
    prof = (sp, utc, c.t0, 64, 64)
    for ad, rule in (((bad(dur, 9, -1), par, unit), 9), ((dur, bad(par, 11, -5), unit), 11),
                     ((dur, par, bad(unit, 20, 0)), 20), ((bad(dur, 3, 77_000), par, unit), 3),
                     ((dur, bad(par, 1, 3), unit), 1)):
        e1 = code(eng.expand_verdicts, *args, ad, None)
        e2 = code(eng.admit, *prof, *ad)
        assert e1.code == e2.code == _lib.CG_EINVAL and f"rule {rule}:" in e1.msg and f"rule {rule}:" in e2.msg
        assert e1.msg.split(": ", 1)[1] == e2.msg.split(": ", 1)[1]
    e1 = code(eng.expand_verdicts, *args, (bad(dur, 0, 60_000), bad(par, 0, 17), None), None)
    assert e1.code == _lib.CG_ERANGE and "rule 0:" in e1.msg
    for lk, rule in (((bad(kind, 6, 3), avg, lunit, contends), 6), ((kind, avg, bad(lunit, 20, 0), contends), 20),
                     ((kind, bad(avg, 3, 77), lunit, contends), 3)):
        e1 = code(eng.expand_verdicts, *args, None, lk + (300,))
        e2 = code(eng.lock_runs, *prof, *lk)
        assert e1.code == e2.code == _lib.CG_EINVAL and f"rule {rule}:" in e1.msg and f"rule {rule}:" in e2.msg
    assert code(eng.expand_verdicts, *args, None, (kind, avg, lunit, contends, 1)).code == _lib.CG_EINVAL
    assert code(eng.expand_verdicts, *args, None, None).code == _lib.CG_EINVAL
    assert code(eng.expand_verdicts, sp, utc, c.t1, c.t0, admit, None).code == _lib.CG_EINVAL
    assert code(eng.expand_verdicts, sp, utc, c.t0, c.t0 + _lib.MAX_HORIZON + 1, admit, None).code == _lib.CG_ERANGE
    # ... and the previous results stayed readable
    same("still readable", c.off, eng.verdicts_copy(0, len(a)), a)
    assert eng.result_device()[2] == len(a)

    # a stuck rule (Apia's skipped day): cg_expand_device's message, no verdicts readable
    scheds = [cron.Parse(s) for s in ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]]
    apia = product_zone("Pacific/Apia")
    ta = 1325030400
    e1 = code(eng.expand, scheds, apia, ta, ta + 5 * 86400)
    e2 = code(eng.expand_verdicts, scheds, apia, ta, ta + 5 * 86400, ([7_200_000] * 3, [1] * 3, None), None)
    assert e1.code == e2.code == _lib.CG_ERANGE and e2.msg == e1.msg
    assert code(eng.verdicts_device).code == _lib.CG_EINVAL
    # a granted fire whose Next never returns: the lock profile's refusal
    tl = 1323907217
    e2 = code(eng.expand_verdicts, scheds, apia, tl, tl + 96 * 3600, None, ([1] * 3, [1000] * 3, None, None, 300))
    e3 = code(eng.lock_runs, scheds, apia, tl, 3600, 96, [1] * 3, [1000] * 3)
    assert e2.code == e3.code == _lib.CG_ERANGE and "rule 1:" in e2.msg and "rule 1:" in e3.msg
    assert code(eng.verdicts_device).code == _lib.CG_EINVAL

    # after a later expand_device the accessors refuse, result_device serves the new result
    n = eng.expand_verdicts_device(sp, utc, c.t0, c.t1, admit, lock)
    eng.verdicts_select(3, 3)
    n2 = eng.expand_device(sp, utc, c.t0, c.t0 + 100)
    assert n2 < n and eng.result_device()[2] == n2
    for fn, a_ in ((eng.verdicts_device, ()), (eng.verdicts_copy, (0, 1)), (eng.verdicts_select, (1, 1)),
                   (eng.verdicts_selected_device, ())):
        assert code(fn, *a_).code == _lib.CG_EINVAL
    # ... and so after a count or a profile call, which rewrite the offsets the bytes index
    eng.expand_verdicts_device(sp, utc, c.t0, c.t1, admit, lock)
    eng.profile(sp, utc, c.t0, 64, 64)
    assert code(eng.verdicts_device).code == _lib.CG_EINVAL
    same("a fresh call", c.off, eng.expand_verdicts(sp, utc, c.t0, c.t1, admit, lock)[2], a)
    sp.free()


# ------------------------------------------------------------------ job set --
def the_jobs():
    """12 jobs on 5 nodes in 2 groups: alone, interval and common kinds, one job
    whose rules differ in node membership (split), one paused, one that repeats
    a Cmd key."""
    groups = {"g1": Group("g1", "g", ["n1", "n2"]), "g2": Group("g2", "h", ["n3", "n4", "n0"])}

    def job(i, kind, avg, rules, **kw):
        return Job(ID=f"job{i:02d}", Kind=kind, AvgTime=avg,
                   Rules=[JobRule(ID=m.pop("ID", f"r{i}.{k}"), Timer=t, **m) for k, (t, m) in enumerate(rules)], **kw)
    on = lambda *n, **kw: dict({"NodeIDs": list(n)}, **kw)  # noqa: E731
    jobs = [
        job(0, KindAlone, 2500, [("@every 60s", on("n0", "n1", "n2"))]),
        job(1, KindCommon, 25_000, [("*/10 * * * * *", on("n0", "n1")), ("*/15 * * * * *", on("n0", "n1"))],
            Parallels=2),
        job(2, KindInterval, 0, [("0 0,1 * * * *", on("n3"))]),
        job(3, KindInterval, 10_000, [("0 * * * * *", on("n0")), ("30 * * * * *", {"GroupIDs": ["g1"]})],
            Parallels=1),  # rules differ in node membership: split
        job(4, KindCommon, 90_000, [("*/20 * * * * *", on("n0", "n3"))], Parallels=1),
        job(5, KindAlone, 45_000, [("*/10 * * * * *", on("n2", "n3")), ("5/10 * * * * *", on("n2", "n3"))]),
        job(6, KindInterval, 0, [("*/7 * * * * *", {"GroupIDs": ["g1"], "ExcludeNodeIDs": ["n1"]})]),
        job(7, KindAlone, 1000, [("* * * * * *", on("n4"))]),
        job(8, KindCommon, 61_000, [("0 * * * * *", on("n1", ID="same")), ("30 * * * * *", on("n1", ID="same"))],
            Parallels=1),  # a repeated Cmd key: the first rule runs nowhere
        job(9, KindInterval, 500, [("@every 90s", on("n2", "n3"))], Pause=True),
        job(10, KindCommon, 200_000, [("15,45 * * * * *", {"GroupIDs": ["g2"]})], Parallels=3),
        job(11, KindCommon, 0, [("@hourly", on("n0", "n1", "n2", "n3", "n4"))]),
    ]
    return jobs, groups


def test_jobset_fire_verdicts_and_node_failures(eng):
    jobs, groups = the_jobs()
    js = JobSet(jobs, groups)
    t0, t1 = PC.T0_UTC, PC.T0_UTC + 5400
    specs = [r.Timer for r in js.rules]
    osch = oracle_parse_all(specs)
    eo, et = O.expand_batch(O.sched_array(osch), t0, t1, oracle_zone("UTC"))
    nodes = ["n0", "n1", "n2", "n3", "n4"]
    index = {id(r): i for i, r in enumerate(js.rules)}
    # the rules each node runs, by the literal Job.Cmds
    runs = {n: sorted(index[id(rule)] for j in jobs for _, rule in j.Cmds(n, groups).values()) for n in nodes}
    contends = np.zeros(len(specs), dtype=np.uint8)
    for n in nodes:
        contends[runs[n]] = 1
    assert not contends[index[id(jobs[8].Rules[0])]] and not contends[index[id(jobs[9].Rules[0])]]
    kind, avg = js.rule_kinds()
    dur, _ = js.rule_durations()
    unit, split = admission_units(js.rules_in())
    assert sorted(jobs[j].ID for j in split) == ["job03", "job08"]
    job_unit = np.asarray(js.rule_job, dtype=np.int32)
    exp = VM.verdicts_from_lists(eo, et, t0, t1, admit=(dur, js.rule_parallels(), unit),
                                 lock=(kind, avg, job_unit, contends), ttl_of=ttl_oracle(osch, "UTC", kind, avg, 300))
    assert (exp & D).any() and (exp & S).any() and (exp == (D | S)).any()
    off, times, v, split_ids = js.fire_verdicts(t0, t1, engine=eng)
    assert split_ids == ["job03", "job08"]
    assert np.array_equal(off, eo)
    same("JobSet times", eo, times, et)
    same("JobSet.fire_verdicts", eo, v, exp)
    names = {D: "dropped", S: "skipped", D | S: "dropped+skipped"}
    rule = np.repeat(np.arange(len(specs)), np.diff(eo))
    for n in ("n0", "n3"):
        want = sorted((int(t), int(r)) + (names[int(x)],) for t, r, x in zip(et, rule, exp) if x and r in runs[n])
        want = [(t, jobs[js.rule_job[r]].ID, js.rules[r].ID, w) for t, r, w in want]
        got = js.node_failures(n, t0, t1, engine=eng)
        assert len(got) == len(want) and len(want) > 0, (n, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"node {n} entry {i}: {g} vs {w}"
    with pytest.raises(KeyError):
        js.node_failures("nope", t0, t1, engine=eng)
