"""Rule sets and oracle expectations shared by the fire-profile tests
(test_gpu_profile.py, test_profile_model.py, test_gpu_profile_scale.py)."""
import zlib

import numpy as np

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, product_zone, random_spec
from cronsun_amd import synth
from cronsun_amd.engine import RulesIn

T0_UTC = 1767571217  # 2026-01-05 00:00:17 UTC

EXTRA = ["* * * * * *", "7,30,45 * * * * *", "0 0 0 29 2 *", "0 0 0 30 Feb ?", "@every 7s", "@every 90m",
         "@every 100h"]


def oracle_profile(oscheds, zone, t0, w, B, chunk=128):
    """rule_counts [R, B] int32 from the oracle's fire lists (a chunk of rules
    at a time, so a dense 98-day horizon never holds every list at once).
    Raises O.NonTerminating with indices into oscheds."""
    R = len(oscheds)
    out = np.zeros((R, B), dtype=np.int32)
    t1 = t0 + B * w
    stuck = []
    for lo in range(0, R, chunk):
        hi = min(R, lo + chunk)
        try:
            off, times = O.expand_batch(O.sched_array(oscheds[lo:hi]), t0, t1, oracle_zone(zone), threads=8)
        except O.NonTerminating as e:
            stuck += [lo + i for i in e.rules]
            continue
        rule = np.repeat(np.arange(hi - lo, dtype=np.int64), np.diff(off))
        cell = rule * B + (times - t0 - 1) // w
        out[lo:hi] = np.bincount(cell, minlength=(hi - lo) * B).reshape(hi - lo, B)
    if stuck:
        raise O.NonTerminating(stuck)
    return out


def oracle_node_matrix(rin, mode, rule_counts):
    roff, rules = O.node_rules(rin, mode, np.arange(rin.n_nodes))
    out = np.zeros((rin.n_nodes, rule_counts.shape[1]), dtype=np.int64)
    for n in range(rin.n_nodes):
        out[n] = rule_counts[rules[roff[n]:roff[n + 1]]].sum(axis=0, dtype=np.int64)
    return out, roff


def utc_specs(max_every_second=None, stride=1, n=777):
    specs = synth.spec_mix(n, every_second_frac=0.01)[::stride] + EXTRA
    if max_every_second is not None:  # the others become hourly rules: R stays
        seen = 0
        for i, s in enumerate(specs):
            if s == "* * * * * *":
                seen += 1
                if seen > max_every_second:
                    specs[i] = "@hourly"
    return specs


def first_transition_2026(zone):
    from test_zone import _table
    when, _ = _table(product_zone(zone), 1767225600, 1798761600)
    return int(when[1])


def zone_specs(zone, n=200):
    """n random valid specs (seeded by the zone) plus an every-second rule and
    an @every."""
    rng = np.random.default_rng(zlib.crc32(("profile" + zone).encode()))
    specs = []
    while len(specs) < n:
        s = random_spec(rng)
        if O.parse(s)[1] is None:
            specs.append(s)
    return specs + ["* * * * * *", "@every 11s"]


def edited(rin, seed):
    """rin with two more nodes -- node N in every rule's NodeIDs (its list
    spans many chunks), node N+1 in none (a zero row) -- and a tenth of the
    jobs paused."""
    N = rin.n_nodes
    R = rin.n_rules
    lens = np.diff(rin.nid_off)
    nid_off = np.concatenate([[0], np.cumsum(lens + 1)]).astype(np.int64)
    nids = np.empty(int(nid_off[-1]), dtype=np.int32)
    for r in range(R):
        a, b = int(rin.nid_off[r]), int(rin.nid_off[r + 1])
        nids[nid_off[r]:nid_off[r] + (b - a)] = rin.nids[a:b]
        nids[nid_off[r + 1] - 1] = N
    pause = np.array(rin.job_pause[:rin.n_jobs], dtype=np.uint8)
    pause[np.random.default_rng(seed).random(rin.n_jobs) < 0.1] = 1
    return RulesIn(N + 2, rin.n_groups, R, rin.n_jobs, rule_key=rin.rule_key,
                   group_off=rin.group_off, group_nodes=rin.group_nodes, group_exists=rin.group_exists,
                   rule_job=rin.rule_job, nid_off=nid_off, nids=nids, gid_off=rin.gid_off, gids=rin.gids,
                   ex_off=rin.ex_off, ex=rin.ex, job_pause=pause)


_sets = {}


def rule_set(name):
    """(rin, specs, oracle schedules), built once per process."""
    if name not in _sets:
        if name == "nodes48":
            # (groups of 4-24 nodes: the default sizes need more than 48 nodes)
            rin = edited(synth.rules_for_nodes(3000, n_nodes=48, n_groups=12, group_size=(4, 24)), 5)
        else:
            rin = edited(synth.multi_rule_jobs(400, n_nodes=64, key_choices=3), 6)
        specs = synth.spec_mix(rin.n_rules, seed=4, mix=synth.MIX_LIGHT)
        _sets[name] = (rin, specs, oracle_parse_all(specs))
    return _sets[name]


# ------------------------------------------------------------- base sets --
class Base:
    """A base set: its specs, t0, zone and the oracle's fire lists over
    (t0, t0 + horizon], from which matrix(w, B) bins any w * B <= horizon."""

    def __init__(self, specs, zone, t0, horizon):
        loc = oracle_zone(zone)
        try:
            self.off, self.times = O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + horizon, loc)
        except O.NonTerminating as e:  # a rule whose loop never ends in this zone: not part of the base
            specs = [s for i, s in enumerate(specs) if i not in set(e.rules)]
            self.off, self.times = O.expand_batch(O.sched_array(oracle_parse_all(specs)), t0, t0 + horizon, loc)
        self.specs, self.zone, self.t0, self.horizon = specs, zone, t0, horizon
        self._m = {}

    @property
    def K(self):
        return len(self.specs)

    def matrix(self, w, B):
        import profile_model as PM
        assert w * B <= self.horizon
        if (w, B) not in self._m:
            self._m[(w, B)] = PM.bin_fires(self.off, self.times, self.t0, w, B)
        return self._m[(w, B)]


UTC_HORIZON = 20 * 4096  # the longest w * B of the scale tests (22 h 45 min)
# 08:59:17: the first minute holds 09:00:00, where hourly and daily rules fire,
# so even one 60-s bucket tells many base rows apart
T0_SCALE = T0_UTC + 9 * 3600 - 60
_bases = {}


def utc_base():
    """About 600 rules of the config-2 mix and EXTRA, three of them
    every-second."""
    if "utc" not in _bases:
        _bases["utc"] = Base(utc_specs(3, n=593), "UTC", T0_SCALE, UTC_HORIZON)
    return _bases["utc"]


def zone_base(zone="Australia/Lord_Howe", w=1800, B=24):
    """About 200 random specs, t0 six hours before the zone's first 2026
    transition, w * B = 12 h across it."""
    if zone not in _bases:
        _bases[zone] = Base(zone_specs(zone), zone, first_transition_2026(zone) - 6 * 3600, w * B)
    return _bases[zone]
