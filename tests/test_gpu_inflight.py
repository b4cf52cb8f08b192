"""In-flight profile on the GPU (cg_inflight_*, cg_profile_node_peaks):
commands running per (rule, bucket edge) and per (node, bucket edge), against
the host model (inflight_model.py: two ranks in the oracle's fire list per
cell) and the oracle's Job.Cmds filter for the per-node matrix.  Exact integer
equality throughout; the first differing (row, bucket) is named.  The oracle's
fire lists are built once per module."""
import numpy as np
import pytest

import inflight_model as IM
import oracle_lib as O
import profile_cases as PC
import profile_model as PM
from common import oracle_zone, product_zone
from cronsun_amd import _lib, cron
from join_cases import nid_rules

pytestmark = pytest.mark.gpu

NY_SPRING, NY_FALL = 1772953200, 1793512800  # 2026-03-08 07:00Z, 2026-11-01 06:00Z
HOUR, DAY = 3600_000, 86400_000  # ms


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


# ---------------------------------------------------------------- helpers --
_bases = {}


def cached(key, make):
    if key not in _bases:
        _bases[key] = make()
    return _bases[key]


def utc_long():
    """utc_base()'s rules over the longest w * B of the UTC cases (3599 x 64,
    past utc_base()'s own 20 x 4096 horizon), from the same t0."""
    b = PC.utc_base()
    return cached("utc_long", lambda: PC.Base(b.specs, "UTC", b.t0, 3599 * 64))


def same(what, got, exp, row="rule"):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        at = [int(x[0]) for x in np.nonzero(got != exp)]
        where = f"{row} {at[0]} bucket {at[1]}" if got.ndim == 2 else f"bucket {at[0]}"
        raise AssertionError(f"{what}: {where}: {int(got[tuple(at)])} vs {int(exp[tuple(at)])}")


def upload(eng, specs):
    return eng.upload([cron.Parse(s) for s in specs])


def check_base(eng, base, w, B, dur, what):
    """Engine.inflight on a base set: the rule matrix equals the model over the
    base's fire lists, the totals its column sums."""
    dur = np.asarray(dur, dtype=np.int64)
    exp = IM.inflight_from_lists(base.off, base.times, base.t0, w, B, IM.seconds(dur))
    sp = upload(eng, base.specs)
    rules, totals = eng.inflight(sp, product_zone(base.zone), base.t0, w, B, dur)
    sp.free()
    same(f"{what} rule matrix", rules, exp)
    same(f"{what} totals", totals, exp.sum(axis=0, dtype=np.int64))
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    return exp


def cycle(values, n):
    return np.array([values[i % len(values)] for i in range(n)], dtype=np.int64)


# ------------------------------------------------------------ rule matrix --
@pytest.mark.parametrize("w,B", [(1, 130), (60, 65), (3599, 64), (20, 4096), (81920, 1)])
def test_rule_matrix_utc(eng, w, B):
    """About 600 rules (every-second, @every delays that divide no width,
    never-firing rules); B below, at and above a wave, the largest B, one
    bucket.  Durations cycle by rule index through 0, 1, 999, 1000, 1001 ms,
    w*1000 - 1, w*1000, w*1000 + 1, 3.5 w, 45 days and INT64_MAX ms."""
    base = utc_long()
    exp = check_base(eng, base, w, B, cycle(IM.duration_cycle(w), base.K), f"UTC w={w} B={B}")
    assert exp.any() and not exp[0::11].any()  # (the rules with 0 ms)


@pytest.mark.parametrize("ms", [HOUR, 35 * DAY, 65 * DAY])
def test_across_segment_cuts(eng, ms):
    """72 rules over 70 days in 10 one-week buckets: the lower edge e - d lies
    in the bucket's own plan segment (1 h), one (35 days) and two (65 days)
    30-day segments back."""
    base = cached("cuts", lambda: PC.Base(PC.utc_specs(0, stride=12), "UTC", PC.T0_UTC, 70 * 86400))
    exp = check_base(eng, base, 604800, 10, np.full(base.K, ms), f"70 days, {ms} ms")
    assert exp.any()


ZONE_DUR = [1000, 29 * 60_000, 30 * 60_000, 31 * 60_000, 5 * HOUR, 13 * HOUR]  # the last: past the 12-h horizon


def zone_case(zone, tau):
    if tau is None:
        return PC.zone_base(zone)
    return cached((zone, tau), lambda: PC.Base(PC.zone_specs(zone), zone, tau - 6 * 3600 + 17, 1800 * 24))


@pytest.mark.parametrize("w,B", [(1800, 24), (37, 1160)])
@pytest.mark.parametrize("zone,tau", [("America/New_York", NY_SPRING), ("America/New_York", NY_FALL),
                                      ("America/Havana", None), ("Australia/Lord_Howe", None),
                                      ("Pacific/Chatham", None)])
def test_rule_matrix_zones(eng, zone, tau, w, B):
    """t0 six hours before a 2026 transition, 12 h across it: bucket edges and
    lower edges inside WALK windows and on the transition instant.  Durations
    of 1 s, 29 | 30 | 31 min (the half-hour buckets), 5 h and more than the
    horizon cycle by rule index; the every-second rule runs 5 h, so inside a
    WALK window its 3600 walked fires an hour stay in flight across hundreds
    of buckets -- the case the two-cursor sweep exists for."""
    base = zone_case(zone, tau)
    dur = cycle(ZONE_DUR, base.K)
    dur[base.specs.index("* * * * * *")] = 5 * HOUR
    exp = check_base(eng, base, w, B, dur, f"{zone} w={w} B={B}")
    every = exp[base.specs.index("* * * * * *")]
    assert every[-1] == min(5 * 3600, w * B) and every[0] == w


# ------------------------------------------- identities, past the grid cap --
def test_identities_past_the_grid_cap(eng):
    """20 011 rules x 65 one-minute buckets = 1.3 M cells, more than the 4096
    blocks x 256 lanes of k_inflight_rules' grid: against Engine.profile of
    the same set -- d = w the start matrix, d = 3 w the 3-bucket sliding sum,
    d = 0 nothing, INT64_MAX ms the prefix sums -- and, with durations a
    function of the base rule, against model[pick]."""
    base = PC.utc_base()
    w, B, R = 60, 65, 20_011
    assert R * B > 4096 * 256
    pick = PM.make_pick(base.K, R, seed=R)
    barr, status = cron.parse_batch(base.specs, threads=8)
    assert not np.any(status)
    a = np.ascontiguousarray(np.ctypeslib.as_array(barr)[:base.K][pick])
    sp = eng.upload_c((barr._type_ * R).from_buffer(a), R)
    utc = product_zone("UTC")
    starts, start_totals = eng.profile(sp, utc, base.t0, w, B)
    same("Engine.profile", starts, base.matrix(w, B)[pick])
    assert eng.profile_kind() == _lib.PROFILE_STARTS

    def call(ms):
        return eng.inflight(sp, utc, base.t0, w, B, np.full(R, ms, dtype=np.int64))
    rules, totals = call(60_000)
    same("d = w", rules, starts)
    same("d = w totals", totals, start_totals)
    rules, totals = call(180_000)
    same("d = 3 w", rules, IM.sliding_sum(starts, 3).astype(np.int32))
    rules, totals = call(0)
    assert not rules.any() and not totals.any()
    rules, totals = call(IM.INT64_MAX)
    pre = np.cumsum(starts, axis=1, dtype=np.int64)
    same("d = INT64_MAX ms", rules, pre.astype(np.int32))
    same("d = INT64_MAX ms totals", totals, pre.sum(axis=0))
    dur_base = cycle(IM.duration_cycle(w), base.K)
    model = IM.inflight_from_lists(base.off, base.times, base.t0, w, B, IM.seconds(dur_base))
    rules, totals = eng.inflight(sp, utc, base.t0, w, B, dur_base[pick])
    same("durations by base rule", rules, model[pick])
    same("durations by base rule, totals", totals, PM.totals(model, pick))
    sp.free()


# ---------------------------------------------------------------- per node --
def set_lists(name):
    """The oracle's fire lists of rule_set(name) over the longest horizon of
    the node cases (65 minutes)."""
    return cached(("lists", name), lambda: O.expand_batch(O.sched_array(PC.rule_set(name)[2]), PC.T0_UTC,
                                                         PC.T0_UTC + 3900, oracle_zone("UTC")))


@pytest.mark.parametrize("w,B", [(60, 65), (600, 6)])
@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
@pytest.mark.parametrize("name", ["nodes48", "keys3"])
def test_node_matrix_and_peaks(eng, name, mode, w, B):
    """3000 one-rule jobs on 48 nodes / 400 jobs whose rules repeat Cmd keys,
    each with a node every rule names (its list spans many chunks), a node no
    rule reaches (a zero row, peak (0, 0)) and paused jobs: every node's row
    equals the oracle's join applied to the model's rule matrix, the peaks are
    each row's max and first argmax -- and the same after a start profile."""
    rin, specs, _ = PC.rule_set(name)
    off, times = set_lists(name)
    t0, N = PC.T0_UTC, rin.n_nodes
    dur = cycle(IM.duration_cycle(w), len(specs))
    exp_rules = IM.inflight_from_lists(off, times, t0, w, B, IM.seconds(dur))
    exp, roff = PC.oracle_node_matrix(rin, mode, exp_rules)
    assert roff[N - 1] - roff[N - 2] > 512 and roff[N] == roff[N - 1]  # the heavy node, the empty one
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    utc = product_zone("UTC")
    got = eng.inflight_per_node(sp, utc, t0, w, B, dur, dr, mode)
    same(f"{name} mode {mode} node matrix", got, exp, "node")
    same("rule matrix", eng.profile_rules(), exp_rules)
    same("totals", eng.profile_totals(), exp_rules.sum(axis=0, dtype=np.int64))
    peak, bucket = eng.profile_node_peaks()
    ep, eb = IM.peaks(exp)
    same("peaks", peak, ep)
    same("peak buckets", bucket, eb)
    assert (peak[N - 1], bucket[N - 1]) == (0, 0) and peak[N - 2] > 0
    p1, b1 = eng.profile_node_peaks(N - 3, 2)  # a range, served from the cached peaks
    assert p1.tolist() == ep[N - 3:N - 1].tolist() and b1.tolist() == eb[N - 3:N - 1].tolist()
    # ... and the peaks of a start profile
    starts = PM.bin_fires(off, times, t0, w, B)
    exp_s = PC.oracle_node_matrix(rin, mode, starts)[0]
    same("start node matrix", eng.profile_per_node(sp, utc, t0, w, B, dr, mode), exp_s, "node")
    assert eng.profile_kind() == _lib.PROFILE_STARTS
    peak, bucket = eng.profile_node_peaks()
    same("start peaks", peak, IM.peaks(exp_s)[0])
    same("start peak buckets", bucket, IM.peaks(exp_s)[1])
    assert not np.array_equal(exp_s, exp)
    dr.free()
    sp.free()


@pytest.mark.parametrize("w,B,row", [(600, 6, [1, 0, 1, 0, 0, 0]), (60, 130, None)])
def test_peak_tie_goes_to_the_first_bucket(eng, w, B, row):
    """Rules firing once, each running exactly one width, on one node: equal
    peaks in different buckets.  B = 6: buckets 0 and 2 (two lanes of the
    wave).  B = 130: buckets 4, 24 and 68 (68 = 4 + 64: the same lane's second
    trip, and another lane).  The second node runs nothing."""
    specs = ["0 5 0 * * *", "0 25 0 * * *", "0 9 1 * * *"]
    rin = nid_rules(2, [[0], [0], [0]])
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    got = eng.inflight_per_node(sp, product_zone("UTC"), PC.T0_UTC, w, B, [w * 1000] * 3, dr, _lib.EXCLUDE_NONE)
    if row is None:
        row = [int(b in (4, 24, 68)) for b in range(B)]
    assert got.tolist() == [row, [0] * B]
    peak, bucket = eng.profile_node_peaks()
    assert peak.tolist() == [1, 0] and bucket.tolist() == [row.index(1), 0]
    assert peak.dtype == np.int64 and bucket.dtype == np.int32
    dr.free()
    sp.free()


# ------------------------------------------------------------------- state --
def test_state_between_calls(eng):
    """profile_kind flips; a start profile after an in-flight call returns
    starts and the reverse; a refused in-flight call (Apia's skipped day)
    leaves nothing readable and the next call is exact; a negative duration is
    refused before anything changes; no rule is valid."""
    base = PC.utc_base()
    w, B, K = 60, 65, base.K
    utc = product_zone("UTC")
    sp = upload(eng, base.specs)
    starts = base.matrix(w, B)
    dur = cycle(IM.duration_cycle(w), K)
    model = IM.inflight_from_lists(base.off, base.times, base.t0, w, B, IM.seconds(dur))
    assert not np.array_equal(model, starts)
    same("in flight", eng.inflight(sp, utc, base.t0, w, B, dur)[0], model)
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    same("starts after in flight", eng.profile(sp, utc, base.t0, w, B)[0], starts)
    assert eng.profile_kind() == _lib.PROFILE_STARTS
    same("in flight after starts", eng.inflight(sp, utc, base.t0, w, B, dur)[0], model)
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    with pytest.raises(_lib.CgError):  # no node matrix: no peaks
        eng.profile_node_peaks()

    # a negative duration: CG_EINVAL naming the rule, the previous profile still readable
    bad = dur.copy()
    bad[[7, 300]] = -1
    with pytest.raises(_lib.CgError) as e:
        eng.inflight(sp, utc, base.t0, w, B, bad)
    assert e.value.code == _lib.CG_EINVAL and "rule 7:" in e.value.msg
    with pytest.raises(_lib.CgError) as e:
        _lib.check(_lib.lib().cg_inflight_device(eng._h, sp._h, eng._loc(utc).handle, base.t0, w, B, None))
    assert e.value.code == _lib.CG_EINVAL
    with pytest.raises(ValueError):
        eng.inflight(sp, utc, base.t0, w, B, dur[:-1])
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    same("still readable", eng.profile_rules(), model)

    # Apia across the skipped 2011-12-30: the message of Engine.expand, nothing readable
    specs = ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]
    scheds = [cron.Parse(s) for s in specs]
    apia = product_zone("Pacific/Apia")
    t0 = 1325030400
    with pytest.raises(_lib.CgError) as e1:
        eng.expand(scheds, apia, t0, t0 + 5 * 86400)
    with pytest.raises(_lib.CgError) as e2:
        eng.inflight(scheds, apia, t0, 3600, 120, [HOUR] * 3)
    assert e1.value.code == e2.value.code == _lib.CG_ERANGE
    assert e2.value.msg == e1.value.msg and "rule 1:" in e2.value.msg
    for read in (eng.profile_totals, eng.profile_kind):
        with pytest.raises(_lib.CgError):
            read()
    same("after the refusal", eng.inflight(sp, utc, base.t0, w, B, dur)[0], model)

    # no rule: valid, an empty matrix and zero totals
    rules, totals = eng.inflight(sp.slice(0, 0), utc, base.t0, w, 24, [])
    assert rules.shape == (0, 24) and totals.shape == (24,) and not totals.any()
    assert eng.profile_kind() == _lib.PROFILE_INFLIGHT
    sp.free()


def test_per_node_call_shares_the_join_cache(eng):
    """An in-flight per-node call reuses the join a start-profile call on the
    same rule set and mode left, and leaves it for the next."""
    rin, specs, _ = PC.rule_set("keys3")
    off, times = set_lists("keys3")
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    utc = product_zone("UTC")
    w, B = 60, 65
    dur = cycle(IM.duration_cycle(w), len(specs))
    eng.profile_per_node(sp, utc, PC.T0_UTC, w, B, dr, _lib.EXCLUDE_RULE)
    assert eng.profile_kernel_times()[3] > 0  # the join was built
    got = eng.inflight_per_node(sp, utc, PC.T0_UTC, w, B, dur, dr, _lib.EXCLUDE_RULE)
    assert eng.profile_kernel_times()[3] == 0  # ... and reused
    exp_rules = IM.inflight_from_lists(off, times, PC.T0_UTC, w, B, IM.seconds(dur))
    same("node matrix on the cached join", got, PC.oracle_node_matrix(rin, _lib.EXCLUDE_RULE, exp_rules)[0], "node")
    eng.profile_per_node(sp, utc, PC.T0_UTC, w, B, dr, _lib.EXCLUDE_RULE)
    assert eng.profile_kernel_times()[3] == 0
    rules_t, totals_t, nodes_t = eng.inflight_per_node_device(sp, utc, PC.T0_UTC, w, B, dur, dr, _lib.EXCLUDE_RULE)
    assert np.array_equal(nodes_t.cpu().numpy(), got) and np.array_equal(rules_t.cpu().numpy(), exp_rules)
    # the device views of the rule-matrix call are the same numbers
    rules_t, totals_t = eng.inflight_device(sp, utc, PC.T0_UTC, w, B, dur)
    assert np.array_equal(rules_t.cpu().numpy(), exp_rules)
    assert np.array_equal(totals_t.cpu().numpy(), exp_rules.sum(axis=0, dtype=np.int64))
    dr.free()
    sp.free()
