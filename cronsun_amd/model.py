"""cronsun's Job / JobRule / Group model (job.go:38-84, group.go:17-22) and
its rule -> node resolution, on top of the C++ host interning in
libcronsun_gpu.so (cg_jobset_*).

  JobRule.Valid()                  job.go:291-308
  Job.Cmds(nid, groups)            job.go:591-614  (ExcludeNodeIDs is a no-op there)
  Job.IsRunOn(nid, groups)         job.go:616-630
  Job.GetJobNodes(groups)          web/job.go:222-257 (cumulative excludes)
  JobSet.lock_ttls(now, loc)       Cmd.lockTtl (job.go:194-233) for every rule
  JobSet.node_profile(t0, width, n_buckets)
                                   fires per node and bucket ahead of time
  JobSet.node_inflight(t0, width, n_buckets)
                                   commands running per node at each bucket
                                   edge, by each job's AvgTime
  JobSet.node_drops(t0, width, n_buckets)
                                   fires Job.limit() would drop per node and
                                   bucket, by each job's Parallels and AvgTime
  JobSet.node_lock_skips(t0, width, n_buckets)
                                   fires per node and bucket at which a
                                   KindAlone / KindInterval job ran nowhere
  JobSet.job_lock_runs(t0, width, n_buckets)
                                   per exclusive job: its cluster-wide runs
                                   and skipped fires per bucket
  JobSet.node_peak_rules(t0, width, n_buckets, k)
                                   per node: its peak, the bucket, and the k
                                   rules that contribute most to it
  JobSet(jobs, groups)             all jobs interned at once -> RulesIn for the
                                   GPU per-node expansion (node/node.go:121-158
                                   for every node at once)
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from ._lib import check, lib
from .cron import Parse, ParseError, Schedule
from .engine import RulesIn

KindCommon, KindAlone, KindInterval = 0, 1, 2


class ErrNilRule(ValueError):
    """errors.go:19 -- a JobRule with an empty timer."""


@dataclass
class Group:
    ID: str
    Name: str = ""
    NodeIDs: List[str] = field(default_factory=list)

    def Included(self, nid):  # group.go:111-119
        return nid in self.NodeIDs


@dataclass
class JobRule:
    ID: str
    Timer: str = ""
    GroupIDs: List[str] = field(default_factory=list)
    NodeIDs: List[str] = field(default_factory=list)
    ExcludeNodeIDs: List[str] = field(default_factory=list)
    Schedule: Optional[Schedule] = None

    def Valid(self):
        """job.go:291-308: parse Timer into Schedule once."""
        if self.Schedule is not None:
            return None
        if len(self.Timer) == 0:
            raise ErrNilRule("invalid job rule, empty timer.")
        try:
            self.Schedule = Parse(self.Timer)
        except ParseError as e:
            raise ParseError(f"invalid JobRule[{self.Timer}], parse err: {e}") from None
        return None


GroupMap = Dict[str, Group]  # Job has a field named Group


@dataclass
class Job:
    ID: str
    Name: str = ""
    Group: str = ""
    Command: str = ""
    User: str = ""
    Rules: List[JobRule] = field(default_factory=list)
    Pause: bool = False
    Timeout: int = 0
    Parallels: int = 0
    Retry: int = 0
    Interval: int = 0
    Kind: int = KindCommon
    AvgTime: int = 0  # ms, job.go:62 (updated by Job.avgTime, job.go:579-589)

    def ValidRules(self):  # job.go:683-690
        for r in self.Rules:
            r.Valid()

    def Cmds(self, nid, gs: GroupMap):
        """job.go:591-614 -> {Job.ID + Rule.ID: (job, rule)}"""
        js = JobSet([self], gs)
        idx = js.cmds(0, nid)
        return {self.ID + js.rules[i].ID: (self, js.rules[i]) for i in idx}

    def IsRunOn(self, nid, gs: GroupMap):
        return JobSet([self], gs).is_run_on(0, nid)

    def GetJobNodes(self, gs: GroupMap):
        return JobSet([self], gs).job_nodes(0)


def _cstr_array(strs):
    enc = [s.encode() for s in strs]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    return arr, len(enc), enc


class _Interned:
    """Host-side queries over an interned cg_jobset handle (self._h)."""

    def rules_in(self) -> RulesIn:
        """Copy the interned arrays into a RulesIn (numpy-owned)."""
        return rules_in_of(self._h)

    def node_index(self, nid):
        return lib().cg_jobset_node_index(self._h, nid.encode())

    def node_id(self, idx):
        v = lib().cg_jobset_node_id(self._h, idx)
        return None if v is None else v.decode()

    def cmds(self, job, nid):
        out = np.zeros(max(self.n_rules, 1), dtype=np.int32)
        k = check(lib().cg_jobset_cmds(self._h, job, nid.encode(), out.ctypes.data, len(out)))
        return [int(x) for x in out[:k]]

    def is_run_on(self, job, nid):
        return bool(check(lib().cg_jobset_is_run_on(self._h, job, nid.encode())))

    def job_nodes(self, job):
        cap = 1 << 16
        out = np.zeros(cap, dtype=np.int32)
        k = check(lib().cg_jobset_job_nodes(self._h, job, out.ctypes.data, cap))
        return [self.node_id(int(x)) for x in out[:min(k, cap)]]

    def __del__(self):
        try:
            lib().cg_jobset_free(self._h)
        except Exception:
            pass


class JobSet(_Interned):
    """All jobs + groups interned by the C++ host layer (cg_jobset)."""

    def __init__(self, jobs, groups: GroupMap):
        L = lib()
        h = C.c_void_p()
        check(L.cg_jobset_new(C.byref(h)))
        self._h = h
        self.jobs = list(jobs)
        self.groups: GroupMap = dict(groups)
        self.rules: List[JobRule] = []
        self.rule_job: List[int] = []
        for gid, g in groups.items():
            arr, n, keep = _cstr_array(g.NodeIDs)
            check(L.cg_jobset_add_group(h, gid.encode(), C.cast(arr, C.c_void_p), n))
        for ji, j in enumerate(self.jobs):
            check(L.cg_jobset_add_job(h, j.ID.encode(), 1 if j.Pause else 0))
            for r in j.Rules:
                g, ng, k1 = _cstr_array(r.GroupIDs)
                nn_, nnn, k2 = _cstr_array(r.NodeIDs)
                ex, ne, k3 = _cstr_array(r.ExcludeNodeIDs)
                check(L.cg_jobset_add_rule(h, r.ID.encode(), C.cast(g, C.c_void_p), ng,
                                           C.cast(nn_, C.c_void_p), nnn, C.cast(ex, C.c_void_p), ne))
                self.rules.append(r)
                self.rule_job.append(ji)

    @property
    def n_rules(self):
        return len(self.rules)

    def lock_ttls(self, now, loc=None, lock_ttl=300, engine=None):
        """Cmd.lockTtl for every (job, rule) Cmd at time `now` (unix seconds):
        the etcd lease TTL newLock would take (job.go:235-241), 0 for a rule
        that never fires.  lock_ttl = conf.Config.LockTtl."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind = np.array([self.jobs[j].Kind for j in self.rule_job], dtype=np.int32)
        avg = np.array([self.jobs[j].AvgTime for j in self.rule_job], dtype=np.int64)
        return eng.lock_ttl_batch(self.schedules(), loc, now, kind, avg, lock_ttl)

    def node_profile(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None):
        """Commands started per node and bucket over n_buckets buckets of
        `width` seconds from t0 (Engine.profile_per_node): {node ID: int64
        [n_buckets]} -- the load each cronnode's own Cron (node/node.go:121-158,
        node/cron/cron.go:210-275) is about to take, before anything has run
        (the reference only has the executed-jobs statistics, web/info.go:14-22)."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        specs = eng.upload(self.schedules())
        drules = eng.upload_rules(rin)
        try:
            counts = eng.profile_per_node(specs, loc, t0, width, n_buckets, drules, mode)
        finally:
            drules.free()
            specs.free()
        return {self.node_id(n): counts[n] for n in range(rin.n_nodes)}

    def rule_durations(self):
        """(dur_ms int64 [n_rules], rules without an estimate): each rule's
        job's AvgTime, with AvgTime <= 0 (never run, or the reference's
        negative values) counted as 0."""
        return durations_of(np.array([self.jobs[j].AvgTime for j in self.rule_job], dtype=np.int64))

    def rule_parallels(self):
        """int64 [n_rules]: each rule's job's Parallels after alone()
        (job.go:378-387: a KindAlone job runs one instance), negative values
        counted as 0 (unlimited, as Job.limit's `Parallels > 0` treats them)."""
        par = [1 if self.jobs[j].Kind == KindAlone else self.jobs[j].Parallels for j in self.rule_job]
        return np.maximum(np.array(par, dtype=np.int64), 0)

    def node_drops(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None, what="dropped"):
        """Fires Job.limit() would drop per node and bucket
        (Engine.admit_per_node; what="admitted": those it lets run), each
        command running for its job's AvgTime and limited by the job's
        Parallels after alone(): ({node ID: int64 [n_buckets]}, the IDs of
        the jobs that were split).  A job whose rules all have the same node
        membership is one unit: its rules share the limit, as they share the
        job's Count on a node.  A job whose rules differ in NodeIDs, GroupIDs
        or (under an exclude mode) ExcludeNodeIDs, or repeat a Cmd key, is
        split: each of its rules is limited on its own, which over-admits,
        and its ID is returned.  Commands started at or before t0 are not
        known (the first AvgTime over-admits), fires of one second are taken
        in rule order, and the KindAlone / KindInterval locks across nodes
        are node_lock_skips', not this profile's (an alone job is limited per
        node only here)."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        dur, _ = self.rule_durations()
        unit, split = admission_units(rin, mode)
        specs = eng.upload(self.schedules())
        return drops_of(self, eng, specs, rin, t0, width, n_buckets, dur, self.rule_parallels(), unit, loc, mode,
                        what), [self.jobs[j].ID for j in split]

    def node_running(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None):
        """Commands running per node at each bucket edge t0 + (b+1)*width,
        counting only the fires Job.limit() lets start
        (Engine.admit_per_node, what="running"): ({node ID: int64
        [n_buckets]}, the IDs of the jobs that were split).  node_inflight
        less the fires node_drops counts: a job that overruns its period
        shows as Parallels running copies, not as an ever-growing count.
        Durations, limits, units and what is not reproduced are node_drops';
        the job lock is not applied here (job_lock_running)."""
        return self.node_drops(t0, width, n_buckets, loc, mode, engine, what="running")

    def job_lock_running(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """{job ID: int64 [n_buckets]} for the KindAlone / KindInterval jobs,
        cluster-wide: the job's commands running at each bucket edge t0 +
        (b+1)*width, counting only the fires that find the job's lock free
        (Engine.lock_runs, what="running") -- each cluster-wide run once,
        however many nodes the job is scheduled on.  Each run takes the job's
        AvgTime; Parallels of an interval job is not applied.  Taken as
        job_lock_runs, with its limits."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return job_lock_running_of(eng, eng.upload(self.schedules()), self.rules_in(), t0, width, n_buckets, kind,
                                   avg, loc, mode, lock_ttl, lambda j: self.jobs[j].ID)

    def rule_kinds(self):
        """(kind int32 [n_rules], avg_time_ms int64 [n_rules]): each rule's
        job's Kind and AvgTime as stored (Engine.lock_runs' arguments)."""
        return (np.array([self.jobs[j].Kind for j in self.rule_job], dtype=np.int32),
                np.array([self.jobs[j].AvgTime for j in self.rule_job], dtype=np.int64))

    def node_lock_skips(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None,
                        what="skipped"):
        """Fires per node and bucket at which a KindAlone / KindInterval job
        ran on no node, because the job's etcd lock (one key per job, on all
        nodes: job.go:235-271) was still held: {node ID: int64 [n_buckets]}
        (Engine.lock_runs_per_node; what="granted": the fires at which the
        node contends for a free lock -- an upper bound of its runs, since
        which node wins is etcd arrival order).  A job is one unit whatever
        its rules' node membership; a rule that runs on no node under the
        exclude mode, or is replaced everywhere by a later rule with the same
        Cmd key, does not contend.  Each run takes the job's AvgTime and
        lock_ttl is conf.Config.LockTtl.  Locks held at t0 are not known
        (cold start); clock skew, Parallels of an interval job, Retry and the
        arrival order within a second are not reproduced."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return lock_skips_of(self, eng, eng.upload(self.schedules()), self.rules_in(), t0, width, n_buckets, kind, avg,
                             loc, mode, lock_ttl, what)

    def job_lock_runs(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """{job ID: (granted int64 [n_buckets], skipped int64 [n_buckets])}
        for the KindAlone / KindInterval jobs, cluster-wide: the fires at which
        the job runs (once, on whichever node wins the lock) and those at which
        it runs nowhere -- the host sum of the job's rule rows of
        Engine.lock_runs.  Limits as node_lock_skips."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return job_lock_runs_of(eng, eng.upload(self.schedules()), self.rules_in(), t0, width, n_buckets, kind, avg,
                                loc, mode, lock_ttl, lambda j: self.jobs[j].ID)

    def fire_verdicts(self, t0, t1, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """Every fire of every rule over (t0, t1] with its verdict
        (Engine.expand_verdicts): (offsets int64 [R+1], times int64 [E],
        verdict uint8 [E], the IDs of the jobs that were split).  Bit 0
        (_lib.VERDICT_DROPPED): Job.limit() would drop the fire -- a failure
        notice; bit 1 (_lib.VERDICT_SKIPPED): the job's KindAlone /
        KindInterval lock is still held and the job runs on no node.  The
        arguments are node_drops' (rule_durations, rule_parallels,
        admission_units: a split job's rules are limited one by one) and
        node_lock_skips' (rule_kinds, lock_units, Engine.rule_contends); the
        two bits are independent and inherit those profiles' limits."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        off, times, verdict, split = fire_verdicts_of(self, eng, rin, t0, t1, loc, mode, lock_ttl)
        return off, times, verdict, [self.jobs[j].ID for j in split]

    def node_failures(self, nid, t0, t1, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """The fires of node nid's Cmds over (t0, t1] that will not run:
        [(time, job ID, rule ID, "dropped" | "skipped" | "dropped+skipped"),
        ...] in (time, rule) order -- the selection of the fires with a verdict
        bit set (Engine.verdicts_select), restricted on the host to the rules
        the node runs under the exclude mode.  Limits as fire_verdicts."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        n = self.node_index(nid)
        if n < 0:
            raise KeyError(f"unknown node {nid!r}")
        rn_off, rn_nodes = eng.rule_nodes(rin, mode)
        rule_of_pair = np.repeat(np.arange(rin.n_rules), np.diff(rn_off))
        mine = np.unique(rule_of_pair[rn_nodes == n])
        fire_verdicts_of(self, eng, rin, t0, t1, loc, mode, lock_ttl)
        # one selection per bit; a fire in both lists carries both
        what = {}
        for mask, name in ((_lib.VERDICT_DROPPED, "dropped"), (_lib.VERDICT_SKIPPED, "skipped")):
            sel_off, sel_times = eng.verdicts_select(mask, mask)
            for r in mine.tolist():
                for t in sel_times[int(sel_off[r]):int(sel_off[r + 1])].tolist():
                    what[(t, r)] = what[(t, r)] + "+" + name if (t, r) in what else name
        return [(t, self.jobs[self.rule_job[r]].ID, self.rules[r].ID, what[(t, r)]) for t, r in sorted(what)]

    def node_inflight(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None):
        """Commands running per node at each bucket edge t0 + (b+1)*width
        (Engine.inflight_per_node), each rule running for its job's AvgTime
        (job.go:62): ({node ID: int64 [n_buckets]}, the number of rules that
        had no estimate and so count as never in flight).  Commands started at
        or before t0 are not counted and every fire is counted: the fires
        Job.limit() would drop are node_drops', those the KindAlone /
        KindInterval locks skip node_lock_skips'."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        dur, missing = self.rule_durations()
        specs = eng.upload(self.schedules())
        drules = eng.upload_rules(rin)
        try:
            counts = eng.inflight_per_node(specs, loc, t0, width, n_buckets, dur, drules, mode)
        finally:
            drules.free()
            specs.free()
        return {self.node_id(n): counts[n] for n in range(rin.n_nodes)}, missing

    def node_peak_rules(self, t0, width, n_buckets, k=10, inflight=False, loc=None, mode=_lib.EXCLUDE_NONE,
                        engine=None, running=False):
        """Which rules make up each node's peak: {node ID: (peak, bucket,
        [(job ID, rule ID, count), ...])} -- the largest cell of the node's
        row in the profile of node_profile (inflight=True: of node_inflight),
        the first bucket that reaches it, and the node's rules with a count >
        0 in that bucket, ordered by (count descending, rule order ascending)
        and cut to k (at most _lib.TOP_RULES_MAX).  A node that runs nothing
        gives (0, 0, []).  With inflight=True the durations come from
        rule_durations() and the result is (that dict, rules without an
        estimate), as node_inflight.  With running=True the profile is
        node_running's (in flight after Job.limit()) and the result is (that
        dict, the IDs of the jobs that were split)."""
        from .engine import default_engine
        eng = engine or default_engine()
        if inflight and running:
            raise ValueError("inflight and running are two profiles: choose one")
        rin = self.rules_in()
        dur, missing = self.rule_durations() if inflight or running else (None, 0)
        unit, split = admission_units(rin, mode) if running else (None, [])
        res = peak_rules_of(self, eng, eng.upload(self.schedules()), rin, t0, width, n_buckets, k, dur,
                            loc, mode, lambda j: self.jobs[j].ID, lambda r: self.rules[r].ID,
                            (self.rule_parallels(), unit) if running else None)
        if running:
            return res, [self.jobs[j].ID for j in split]
        return (res, missing) if inflight else res

    def schedules(self):
        """Parsed schedules in rule order (JobRule.Valid on each)."""
        for r in self.rules:
            r.Valid()
        return [r.Schedule for r in self.rules]


def durations_of(avg_ms):
    """Per-rule AvgTime (ms) -> (the in-flight profile's dur_ms, how many rules
    have no estimate): AvgTime <= 0 counts as 0."""
    avg = np.asarray(avg_ms, dtype=np.int64)
    return np.maximum(avg, 0), int((avg <= 0).sum())


def admission_units(rin, mode=_lib.EXCLUDE_NONE):
    """(unit int32 [R], split job indices) for Engine.admit*: unit[r] is the
    rule's job index where all rules of the job have the same node membership
    -- the same interned NodeIDs, GroupIDs and, unless mode is EXCLUDE_NONE,
    ExcludeNodeIDs, as sets, and no repeated Cmd key -- so every node the job
    runs on sees all its rules.  The rules of any other job become units of
    their own (numbered past the job indices) and the job is reported."""
    R, J = rin.n_rules, rin.n_jobs
    rule_job = np.asarray(rin.rule_job[:R], dtype=np.int64)
    if R > 1 and (np.diff(rule_job) < 0).any():
        raise ValueError("the rules of a job must be contiguous and the jobs in order")

    def members(off, vals, r):
        return frozenset(np.asarray(vals[int(off[r]):int(off[r + 1])]).tolist())
    unit = np.zeros(R, dtype=np.int64)
    split, nxt = [], J
    cuts = [0] + (np.nonzero(np.diff(rule_job))[0] + 1).tolist() + [R] if R else [0]
    for a, b in zip(cuts[:-1], cuts[1:]):
        sig = {(members(rin.nid_off, rin.nids, r), members(rin.gid_off, rin.gids, r),
                members(rin.ex_off, rin.ex, r) if mode != _lib.EXCLUDE_NONE else None) for r in range(a, b)}
        keys = None if rin.rule_key is None else np.asarray(rin.rule_key[a:b])
        if len(sig) == 1 and (keys is None or len(set(keys.tolist())) == b - a):
            unit[a:b] = rule_job[a]
        else:
            split.append(int(rule_job[a]))
            unit[a:b] = np.arange(nxt, nxt + (b - a))
            nxt += b - a
    # units must not decrease along the rules: renumber in order of appearance
    if R:
        change = np.concatenate([[0], (np.diff(unit) != 0).astype(np.int64)])
        unit = np.cumsum(change)
    return unit.astype(np.int32), split


def drops_of(js, eng, specs, rin, t0, width, n_buckets, dur, par, unit, loc, mode, what):
    """node_drops of a job set: {node ID: int64 [B]} of the per-node admission profile."""
    drules = eng.upload_rules(rin)
    try:
        counts = eng.admit_per_node(specs, loc, t0, width, n_buckets, dur, par, unit, drules, mode, what)
    finally:
        drules.free()
        specs.free()
    return {js.node_id(n): counts[n] for n in range(rin.n_nodes)}


def lock_units(rin):
    """int32 [R] for Engine.lock_runs*: the job index per rule.  The lock key
    is the job's ID, so a job is one unit whatever its rules' node membership
    (unlike admission_units).  The rules of a job must be contiguous and the
    jobs in order."""
    unit = np.asarray(rin.rule_job[:rin.n_rules], dtype=np.int32)
    if unit.size > 1 and (np.diff(unit) < 0).any():
        raise ValueError("the rules of a job must be contiguous and the jobs in order")
    return np.ascontiguousarray(unit)


def lock_skips_of(js, eng, specs, rin, t0, width, n_buckets, kind, avg, loc, mode, lock_ttl, what):
    """node_lock_skips of a job set: {node ID: int64 [B]} of the per-node lock profile."""
    try:
        contends = eng.rule_contends(rin, mode)
        drules = eng.upload_rules(rin)
        try:
            counts = eng.lock_runs_per_node(specs, loc, t0, width, n_buckets, kind, avg, lock_units(rin), contends,
                                            drules, mode, lock_ttl, what)
        finally:
            drules.free()
    finally:
        specs.free()
    return {js.node_id(n): counts[n] for n in range(rin.n_nodes)}


def fire_verdicts_of(js, eng, rin, t0, t1, loc, mode, lock_ttl):
    """fire_verdicts of a job set: (offsets, times, verdict, split job
    indices); the verdicts stay selectable on the engine."""
    dur, _ = js.rule_durations()
    unit, split = admission_units(rin, mode)
    kind, avg = js.rule_kinds()
    contends = eng.rule_contends(rin, mode)
    specs = eng.upload(js.schedules())
    try:
        off, times, verdict = eng.expand_verdicts(specs, loc, t0, t1, admit=(dur, js.rule_parallels(), unit),
                                                  lock=(kind, avg, lock_units(rin), contends, lock_ttl))
    finally:
        specs.free()
    return off, times, verdict, split


def job_lock_runs_of(eng, specs, rin, t0, width, n_buckets, kind, avg, loc, mode, lock_ttl, job_id):
    """job_lock_runs of a job set: per exclusive job the sums of its rules'
    GRANTED and SKIPPED rows."""
    try:
        unit, contends = lock_units(rin), eng.rule_contends(rin, mode)
        rows = [eng.lock_runs(specs, loc, t0, width, n_buckets, kind, avg, unit, contends, lock_ttl, what)[0]
                for what in ("granted", "skipped")]
    finally:
        specs.free()
    out = {}
    for j in np.unique(unit[np.asarray(kind) != KindCommon]).tolist():
        mine = unit == j
        out[job_id(j)] = tuple(r[mine].sum(axis=0, dtype=np.int64) for r in rows)
    return out


def job_lock_running_of(eng, specs, rin, t0, width, n_buckets, kind, avg, loc, mode, lock_ttl, job_id):
    """job_lock_running of a job set: per exclusive job the sum of its rules'
    LOCK_RUNNING rows."""
    try:
        unit, contends = lock_units(rin), eng.rule_contends(rin, mode)
        rows = eng.lock_runs(specs, loc, t0, width, n_buckets, kind, avg, unit, contends, lock_ttl, "running")[0]
    finally:
        specs.free()
    return {job_id(j): rows[unit == j].sum(axis=0, dtype=np.int64)
            for j in np.unique(unit[np.asarray(kind) != KindCommon]).tolist()}


def peak_rules_of(js, eng, specs, rin, t0, width, n_buckets, k, dur, loc, mode, job_id, rule_id, limits=None):
    """node_peak_rules of a job set: the per-node profile (in flight when dur
    is given; running, i.e. in flight after Job.limit(), when limits =
    (parallels, unit) is given too), each node's peak, and its top list at the
    peak bucket mapped back to (job ID, rule ID, count)."""
    drules = eng.upload_rules(rin)
    try:
        if dur is None:
            eng.profile_per_node(specs, loc, t0, width, n_buckets, drules, mode)
        elif limits is not None:
            eng.admit_per_node(specs, loc, t0, width, n_buckets, dur, limits[0], limits[1], drules, mode, "running")
        else:
            eng.inflight_per_node(specs, loc, t0, width, n_buckets, dur, drules, mode)
        peak, _ = eng.profile_node_peaks()
        rule, cnt, n_listed, _, bucket = eng.profile_top_rules(k)
    finally:
        drules.free()
        specs.free()
    out = {}
    for n in range(rin.n_nodes):
        top = [(job_id(int(rin.rule_job[r])), rule_id(int(r)), int(c))
               for r, c in zip(rule[n, :n_listed[n]], cnt[n, :n_listed[n]])]
        out[js.node_id(n)] = (int(peak[n]), int(bucket[n]), top)
    return out


def rules_in_of(h) -> RulesIn:
    """cg_jobset_rules of a handle, copied into a numpy-owned RulesIn."""
    c = _lib.cg_rules_in()
    check(lib().cg_jobset_rules(h, C.byref(c)))

    def arr(ptr, n, dt):
        if n == 0:
            return np.zeros(0, dtype=dt)
        ct = {np.int64: C.c_int64, np.int32: C.c_int32, np.uint8: C.c_uint8}[dt]
        return np.ctypeslib.as_array((ct * n).from_address(ptr)).copy()

    R, G, J = c.n_rules, c.n_groups, c.n_jobs
    nid_off = arr(c.nid_off, R + 1, np.int64)
    gid_off = arr(c.gid_off, R + 1, np.int64)
    ex_off = arr(c.ex_off, R + 1, np.int64)
    group_off = arr(c.group_off, G + 1, np.int64)
    return RulesIn(
        c.n_nodes, G, R, J,
        group_off=group_off, group_nodes=arr(c.group_nodes, int(group_off[-1]), np.int32),
        group_exists=arr(c.group_exists, G, np.uint8), rule_job=arr(c.rule_job, R, np.int32),
        nid_off=nid_off, nids=arr(c.nids, int(nid_off[-1]), np.int32),
        gid_off=gid_off, gids=arr(c.gids, int(gid_off[-1]), np.int32),
        ex_off=ex_off, ex=arr(c.ex, int(ex_off[-1]), np.int32),
        job_pause=arr(c.job_pause, J, np.uint8),
        rule_key=arr(c.rule_key, R, np.int32) if c.rule_key else None)
