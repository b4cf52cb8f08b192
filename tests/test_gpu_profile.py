"""Fire profile on the GPU (cg_profile_*): fires per (rule, bucket) and per
(node, bucket) without the fire lists, against the oracle's literal Next loop
binned with numpy by (t - t0 - 1) // width, and the oracle's Job.Cmds filter
(oracle_lib.node_rules) for the per-node matrix.  Exact integer equality
throughout."""
import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, product_zone
from cronsun_amd import _lib, cron
from profile_cases import (T0_UTC, first_transition_2026, oracle_node_matrix, oracle_profile, rule_set, utc_specs,
                           zone_specs)

pytestmark = pytest.mark.gpu

NY_SPRING, NY_FALL = 1772953200, 1793512800  # 2026-03-08 07:00Z, 2026-11-01 06:00Z


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def check_rules(eng, specs, zone, t0, w, B):
    """The rule matrix equals the oracle's, rows sum to Engine.count, totals
    are the column sums.  Where the oracle's loop never ends for some rule:
    CG_ERANGE naming the first such rule, then the same check without them."""
    scheds = [cron.Parse(s) for s in specs]
    loc = product_zone(zone)
    try:
        exp = oracle_profile(oracle_parse_all(specs), zone, t0, w, B)
    except O.NonTerminating as e:
        with pytest.raises(_lib.CgError) as err:
            eng.profile(scheds, loc, t0, w, B)
        assert err.value.code == _lib.CG_ERANGE
        assert f"rule {e.rules[0]}:" in err.value.msg
        keep = [i for i in range(len(specs)) if i not in set(e.rules)]
        return check_rules(eng, [specs[i] for i in keep], zone, t0, w, B)
    sp = eng.upload(scheds)
    got, totals = eng.profile(sp, loc, t0, w, B)
    assert got.shape == (len(specs), B) and got.dtype == np.int32
    assert totals.shape == (B,) and totals.dtype == np.int64
    if not np.array_equal(got, exp):
        r, b = [int(x[0]) for x in np.nonzero(got != exp)]
        raise AssertionError(f"{zone} t0={t0} w={w} B={B}: rule {r} [{specs[r]}] bucket {b}: "
                             f"{int(got[r, b])} vs {int(exp[r, b])}")
    assert np.array_equal(got.sum(axis=1, dtype=np.int64), eng.count(sp, loc, t0, t0 + B * w))
    assert np.array_equal(totals, exp.sum(axis=0, dtype=np.int64))
    return got, totals


# ------------------------------------------------------------ rule matrix --
@pytest.mark.parametrize("w,B", [(1, 130), (7, 1000), (60, 65), (3599, 64), (3600, 48), (86400, 3), (90000, 1),
                                 (604800, 14), (30, 4096)])
def test_rule_matrix_utc(eng, w, B):
    """784 rules (a multiple of neither a wave nor a block): every-second,
    @every delays that divide no width, rules that never fire; B below, at and
    above a wave, one bucket, the largest B; 98 days over the 30-day segment
    cuts.  The oracle's literal loop walks 0.6-1.6 M fires a second, and the
    784 rules fire 61 M times in 98 days even with the every-second rules
    kept to two (104 s of oracle here): that case takes every twelfth rule of
    the mix and the extras (72 rules, one of them every-second; 13.5 M fires,
    about 10 s of oracle)."""
    specs = utc_specs(2, stride=12) if w * B > 40 * 86400 else utc_specs()
    assert len(specs) % 64 != 0
    check_rules(eng, specs, "UTC", T0_UTC, w, B)


@pytest.mark.parametrize("w,B", [(1800, 24), (37, 1200)])
@pytest.mark.parametrize("zone,tau", [("America/New_York", NY_SPRING), ("America/New_York", NY_FALL),
                                      ("America/Havana", None), ("Australia/Lord_Howe", None),
                                      ("Pacific/Chatham", None)])
def test_rule_matrix_zones(eng, zone, tau, w, B):
    """t0 six hours and 17 s before a 2026 transition: New York's clean
    transitions (the closed form cut at tau - 1), Havana's walked closed-form
    runs, Lord Howe's 30-minute and Chatham's 45-minute-offset shifts; bucket
    edges inside WALK windows and on tau."""
    tau = tau or first_transition_2026(zone)
    specs = zone_specs(zone)
    check_rules(eng, specs, zone, tau - 6 * 3600 + 17, w, B)


def test_apia_skipped_day_is_refused(eng):
    """Pacific/Apia across the skipped 2011-12-30: CG_ERANGE naming the rule
    Engine.expand names; a valid profile call afterwards is exact."""
    specs = ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]
    scheds = [cron.Parse(s) for s in specs]
    apia = product_zone("Pacific/Apia")
    t0 = 1325030400
    with pytest.raises(_lib.CgError) as e1:
        eng.expand(scheds, apia, t0, t0 + 5 * 86400)
    with pytest.raises(_lib.CgError) as e2:
        eng.profile(scheds, apia, t0, 3600, 120)
    assert e1.value.code == e2.value.code == _lib.CG_ERANGE
    assert e2.value.msg == e1.value.msg and "rule 1:" in e2.value.msg
    with pytest.raises(_lib.CgError):  # nothing readable after the failure
        eng.profile_totals()
    check_rules(eng, specs, "Pacific/Apia", t0 - 10 * 86400 + 17, 3600, 120)


# --------------------------------------------------------------- per node --
_oracle_rules = {}


def oracle_rule_matrix(name, w, B):
    if (name, w, B) not in _oracle_rules:
        _oracle_rules[(name, w, B)] = oracle_profile(rule_set(name)[2], "UTC", T0_UTC, w, B)
    return _oracle_rules[(name, w, B)]


@pytest.mark.parametrize("w,B", [(60, 65), (600, 6), (3600, 1), (7, 520)])
@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE])
@pytest.mark.parametrize("name", ["nodes48", "keys3"])
def test_node_matrix(eng, name, mode, w, B):
    """3000 one-rule jobs on 48 nodes / 400 jobs whose rules repeat Cmd keys,
    each with a node every rule names, a node no rule reaches and paused
    jobs: every node's row equals the oracle's join applied to the oracle's
    rule matrix, and the binned lists of Engine.expand_per_node."""
    rin, specs, _ = rule_set(name)
    scheds = [cron.Parse(s) for s in specs]
    utc = product_zone("UTC")
    exp_rules = oracle_rule_matrix(name, w, B)
    exp, roff = oracle_node_matrix(rin, mode, exp_rules)
    N = rin.n_nodes
    assert roff[N - 1] - roff[N - 2] > 512 and roff[N] == roff[N - 1]  # the heavy node, the empty one
    sp, dr = eng.upload(scheds), eng.upload_rules(rin)
    got = eng.profile_per_node(sp, utc, T0_UTC, w, B, dr, mode)
    assert got.shape == (N, B) and got.dtype == np.int64
    if not np.array_equal(got, exp):
        n, b = [int(x[0]) for x in np.nonzero(got != exp)]
        raise AssertionError(f"{name} mode {mode} w={w} B={B}: node {n} bucket {b}: {int(got[n, b])} vs {int(exp[n, b])}")
    assert not got[N - 1].any()
    assert np.array_equal(eng.profile_rules(), exp_rules)
    assert np.array_equal(eng.profile_totals(), exp_rules.sum(axis=0, dtype=np.int64))
    # the per-node lists over the same horizon, binned
    node_off, time, _ = eng.expand_per_node(sp, utc, T0_UTC, T0_UTC + w * B, rin, mode)
    node = np.repeat(np.arange(N, dtype=np.int64), np.diff(node_off))
    binned = np.bincount(node * B + (time - T0_UTC - 1) // w, minlength=N * B).reshape(N, B)
    assert np.array_equal(got, binned)
    dr.free()


def _list_checksums(eng, N):
    o, t, r, n = eng.node_result_device()
    return eng.checksum(o, N + 1, 8), eng.checksum(t, n, 8), eng.checksum(r, n, 4), n


def test_interplay_with_expansion_calls(eng):
    """The per-node profile shares the per-node path's cached join: a list
    call, the profile in the same mode (a hit) and in another (a rebuild),
    the same list call again -- identical lists, identical profile.  After a
    profile the rule-major accessors behave as after Engine.count, and the
    profile survives an intervening expand_device."""
    rin, specs, _ = rule_set("keys3")
    scheds = [cron.Parse(s) for s in specs]
    utc = product_zone("UTC")
    sp, dr = eng.upload(scheds), eng.upload_rules(rin)
    w, B, N = 60, 65, rin.n_nodes
    t1 = T0_UTC + w * B
    a, b = _lib.EXCLUDE_NONE, _lib.EXCLUDE_CUMULATIVE
    eng.expand_per_node_rules_device(sp, utc, T0_UTC, t1, dr, a)
    lists = _list_checksums(eng, N)
    first = eng.profile_per_node(sp, utc, T0_UTC, w, B, dr, a).copy()
    assert eng.profile_kernel_times()[3] == 0  # the cached join was reused
    other = eng.profile_per_node(sp, utc, T0_UTC, w, B, dr, b).copy()
    exp_rules = oracle_rule_matrix("keys3", w, B)
    assert np.array_equal(first, oracle_node_matrix(rin, a, exp_rules)[0])
    assert np.array_equal(other, oracle_node_matrix(rin, b, exp_rules)[0])
    assert not np.array_equal(first, other)
    eng.expand_per_node_rules_device(sp, utc, T0_UTC, t1, dr, a)
    assert _list_checksums(eng, N) == lists
    assert np.array_equal(eng.profile_per_node(sp, utc, T0_UTC, w, B, dr, a), first)

    def rule_major_state():
        out = [eng.result_device()[2]]
        try:
            eng.copy_times(0, 1)
            out.append("ok")
        except _lib.CgError as e:
            out.append((e.code, e.msg))
        return out
    eng.expand_device(sp, utc, T0_UTC, t1)
    eng.count(sp, utc, T0_UTC, t1)
    after_count = rule_major_state()
    eng.expand_device(sp, utc, T0_UTC, t1)
    rules, totals = eng.profile(sp, utc, T0_UTC, w, B)
    assert rule_major_state() == after_count
    # ... and expansion calls leave the profile alone
    E = eng.expand_device(sp, utc, T0_UTC, t1)
    assert E == int(exp_rules.sum())
    assert np.array_equal(eng.profile_rules(), rules) and np.array_equal(eng.profile_totals(), totals)
    assert np.array_equal(rules, exp_rules)
    dr.free()


def test_arguments(eng):
    rin, specs, _ = rule_set("keys3")
    scheds = [cron.Parse(s) for s in specs]
    utc = product_zone("UTC")
    sp, dr = eng.upload(scheds), eng.upload_rules(rin)

    def refused(code, fn, *args):
        with pytest.raises(_lib.CgError) as e:
            fn(*args)
        assert e.value.code == code and e.value.msg
    for fn, tail in ((eng.profile, ()), (eng.profile_per_node, (dr, 0))):
        refused(_lib.CG_EINVAL, fn, sp, utc, T0_UTC, 60, 0, *tail)
        refused(_lib.CG_EINVAL, fn, sp, utc, T0_UTC, 60, 4097, *tail)
        refused(_lib.CG_EINVAL, fn, sp, utc, T0_UTC, 0, 24, *tail)
        refused(_lib.CG_EINVAL, fn, sp, utc, T0_UTC, -5, 24, *tail)
        refused(_lib.CG_ERANGE, fn, sp, utc, T0_UTC, _lib.MAX_HORIZON // 24 + 1, 24, *tail)
    refused(_lib.CG_EINVAL, eng.profile_per_node, sp.slice(0, 10), utc, T0_UTC, 60, 24, dr, 0)
    refused(_lib.CG_EINVAL, eng.profile_per_node, sp, utc, T0_UTC, 60, 24, dr, 3)
    # the longest horizon itself is accepted (two sparse rules)
    few = eng.upload([cron.Parse("@yearly"), cron.Parse("@every 100h")])
    rules, totals = eng.profile(few, utc, T0_UTC, _lib.MAX_HORIZON // 24, 24)
    assert rules[0].sum() == 40 and np.array_equal(totals, rules.sum(axis=0, dtype=np.int64))
    # no rule: valid, zero totals, an empty rule matrix
    rules, totals = eng.profile(sp.slice(0, 0), utc, T0_UTC, 60, 24)
    assert rules.shape == (0, 24) and totals.shape == (24,) and not totals.any()
    # a profile without a per-node call reports no node matrix
    eng.profile(sp, utc, T0_UTC, 60, 24)
    r, t, n, R, N, B = eng.profile_result_device()
    assert r and t and n is None and (R, N, B) == (len(specs), 0, 24)
    out = np.empty(24, dtype=np.int64)
    assert _lib.lib().cg_profile_copy_nodes(eng._h, 0, 1, out.ctypes.data) == _lib.CG_EINVAL
    refused(_lib.CG_EINVAL, eng.profile_rules, len(specs), 1)
    # the device views are the same numbers
    rules_t, totals_t, nodes_t = eng.profile_per_node_device(sp, utc, T0_UTC, 60, 24, dr, 0)
    assert np.array_equal(rules_t.cpu().numpy(), eng.profile_rules())
    assert np.array_equal(totals_t.cpu().numpy(), eng.profile_totals())
    assert np.array_equal(nodes_t.cpu().numpy(), eng.profile_nodes())
    dr.free()
