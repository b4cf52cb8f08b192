"""Lock profile: the API surface that needs no device.  The header declares
the two entry points and the two kinds and states the definition; the ABI
version stays 3; the built library exports the calls, _lib binds them, the
Python surface exists and refuses a bad `what`, a lock_ttl below 2 or a wrong
array shape before any device use; lock_units gives the job index per rule
whatever the rules' membership, contends comes from the join's degrees, and
JobSet / EtcdJobSet hand the jobs' Kind and AvgTime through; the Go stub has
the wrappers; README, DESIGN and the header no longer call the locks
unmodelled and list what remains unreproduced.  Without a device the valid
call is CG_ENODEV."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = {"cg_lock_profile_device": 12, "cg_lock_profile_per_node_device": 14}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_lock_entry_points():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"#define\s+CG_PROFILE_LOCK_GRANTED\s+4\b", txt)
    assert re.search(r"#define\s+CG_PROFILE_LOCK_SKIPPED\s+5\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    # kind, avg_time_ms, unit, contends, lock_ttl, what -- then the rule set and mode in the per-node call
    args = r"n_buckets,\s*const\s+int32_t\s*\*\s*kind\s*,\s*const\s+int64_t\s*\*\s*avg_time_ms\s*,\s*" \
           r"const\s+int32_t\s*\*\s*unit\s*,\s*const\s+uint8_t\s*\*\s*contends\s*,\s*int64_t\s+lock_ttl\s*,\s*int\s+what"
    assert re.search(r"cg_lock_profile_device\s*\([^)]*" + args + r"\s*\)", txt)
    assert re.search(r"cg_lock_profile_per_node_device\s*\([^)]*" + args +
                     r"\s*,\s*const\s+cg_rules\s*\*\s*rules,\s*int\s+mode\s*\)", txt)


def test_header_states_the_definition():
    raw = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    for phrase in ("conf.Config.Lock + Job.ID", "one lock for all rules of the job, on all nodes",
                   "the key lives ttl seconds from the grant", "until ttl seconds after the command ends",
                   "d_r = ceil(max(avg, 0) / 1000)", "does not decrease along r",
                   "differing node membership does not split a unit", "the rule reaches no lock",
                   "time ascending, rule index ascending", "If t < free_at, the fire is SKIPPED",
                   "exactly what cg_lock_ttl_batch returns for now = t", "the state is unchanged",
                   "CG_ERANGE naming the rule and no profile is readable afterwards",
                   "free_at = t + ttl for INTERVAL or t + d_r + ttl for ALONE",
                   "A fire at the very second the lease ends is granted",
                   "granted[r][b] + skipped[r][b] == the start profile",
                   "The SKIPPED node row is exact", "The GRANTED node row is an upper bound",
                   "etcd arrival order", "count each cluster-wide run once",
                   "Locks held at t0 are unknown (cold start)", "Node clock skew", "`now` is taken as t",
                   "Parallels of an INTERVAL job", "limit() is subsumed", "Job.Retry / Interval",
                   "Actual run times differ from AvgTime", "Fires of one second are taken in rule order",
                   "[21] the unit walk (k_lock_units)"):
        assert phrase in raw, phrase


def test_docs_no_longer_call_the_locks_unmodelled():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "cronsun_gpu.h"),
                 os.path.join("cronsun_amd", "model.py"), os.path.join("node", "cron", "gpu", "gpu.go")):
        txt = " ".join(open(os.path.join(ROOT, name)).read().split()).replace(" * ", " ").replace(" // ", " ")
        assert not re.search(r"locks?\b[^.]*\b(are|is) (still )?not modelled", txt, flags=re.I), name
        assert "cg_lock_profile" in txt or "lock_runs" in txt or "LockProfile" in txt, name
    for name in ("README.md", "DESIGN.md"):
        txt = " ".join(open(os.path.join(ROOT, name)).read().split())
        for phrase in ("cg_lock_profile_device", "lock_bench.json", "cold start", "clock skew", "arrival order"):
            assert phrase in txt, (name, phrase)
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("k_lock_units", "lock_walk_unit", "build_lock_table", "lock profile"):
        assert phrase in design, phrase


def test_library_exports_lock_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_lock_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name, arity in NEW.items():
        assert name in _lib.SYMBOLS
        assert len(getattr(L, name).argtypes) == arity, name
    assert (_lib.PROFILE_LOCK_GRANTED, _lib.PROFILE_LOCK_SKIPPED) == (4, 5)
    assert (_lib.JOB_COMMON, _lib.JOB_ALONE, _lib.JOB_INTERVAL) == (0, 1, 2)


def test_python_surface():
    from cronsun_amd import engine, ingest, model
    for m in ("lock_runs", "lock_runs_per_node", "lock_runs_device", "lock_kernel_times", "rule_contends"):
        assert callable(getattr(engine.Engine, m))
    assert callable(model.lock_units) and callable(engine.contends_of)
    for cls in (model.JobSet, ingest.EtcdJobSet):
        assert callable(cls.node_lock_skips) and callable(cls.job_lock_runs) and callable(cls.rule_kinds)


def test_go_stub_has_the_wrappers():
    go = open(os.path.join(ROOT, "node", "cron", "gpu", "gpu.go")).read()
    assert re.search(r"func \(e \*Engine\) LockProfile\(", go)
    assert re.search(r"func \(e \*Engine\) LockProfilePerNode\(", go)
    assert "ProfileLockGranted" in go and "ProfileLockSkipped" in go
    assert "C.cg_lock_profile_device(" in go and "C.cg_lock_profile_per_node_device(" in go


def test_python_refusals_need_no_device():
    """A bad `what`, a lock_ttl below 2 and arrays of the wrong length are
    refused by Engine.lock_runs* before the library is called (no Engine is
    constructed here: the checks are the argument helper's)."""
    from cronsun_amd.engine import Engine
    e = Engine.__new__(Engine)  # no device behind it
    with pytest.raises(ValueError, match="what"):
        e._lock_args(2, [1, 1], [0, 0], None, None, 300, "dropped")
    with pytest.raises(ValueError, match="kind"):
        e._lock_args(2, [1], [0, 0], None, None, 300, "skipped")
    with pytest.raises(ValueError, match="avg_time_ms"):
        e._lock_args(2, [1, 1], [0], None, None, 300, "skipped")
    with pytest.raises(ValueError, match="unit"):
        e._lock_args(2, [1, 1], [0, 0], [0], None, 300, "granted")
    with pytest.raises(ValueError, match="contends"):
        e._lock_args(2, [1, 1], [0, 0], None, [1, 1, 1], 300, "granted")
    with pytest.raises(ValueError, match="lock_ttl"):
        e._lock_args(2, [1, 1], [0, 0], None, None, 1, "granted")
    k, a, u, c, ttl, w = e._lock_args(2, [1, 2], [-5, 2500], [3, 4], [True, 7], 2, "granted")
    assert (k.dtype, a.dtype, u.dtype, c.dtype, ttl, w) == (np.int32, np.int64, np.int32, np.uint8, 2, 4)
    assert c.tolist() == [1, 1] and a.tolist() == [-5, 2500]
    out = e._lock_args(0, [], [], None, None, 300, "skipped")
    assert out[2] is None and out[3] is None and out[5] == 5


def test_null_handles_are_refused_before_any_device_use():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_lock_profile_device(None, None, None, 0, 60, 4, None, None, None, None, 300, 5) == _lib.CG_EINVAL
    assert L.cg_lock_profile_per_node_device(None, None, None, 0, 60, 4, None, None, None, None, 300, 4, None,
                                             0) == _lib.CG_EINVAL


def _jobs():
    from cronsun_amd.model import Group, Job, JobRule, KindAlone, KindInterval
    g = {"g": Group("g", "", ["n0", "n1"]), "h": Group("h", "", ["n1", "n2"])}
    jobs = [
        Job("common", Rules=[JobRule("a", "@every 30s", ["g"], [], []), JobRule("b", "@every 45s", ["g"], [], [])],
            AvgTime=40_000),
        # differing GroupIDs: still one lock unit
        Job("interval", Rules=[JobRule("a", "@every 30s", ["g"], [], []), JobRule("b", "@every 30s", ["h"], [], [])],
            Kind=KindInterval, AvgTime=-7),
        # the second rule repeats the first one's Cmd key and covers its nodes: the first reaches no lock
        Job("alone", Rules=[JobRule("a", "@every 60s", [], ["n0"], []), JobRule("a", "@every 60s", ["g"], [], []),
                            JobRule("c", "@every 60s", [], [], [])],
            Kind=KindAlone, AvgTime=2500),
        Job("paused", Rules=[JobRule("a", "* * * * * *", [], ["n0"], [])], Kind=KindAlone, AvgTime=0, Pause=True),
    ]
    return jobs, g


def _docs():
    jobs, groups = _jobs()
    jd = [json.dumps({"id": j.ID, "kind": j.Kind, "parallels": j.Parallels, "avg_time": j.AvgTime, "pause": j.Pause,
                      "rules": [{"id": r.ID, "timer": r.Timer, "gids": r.GroupIDs, "nids": r.NodeIDs,
                                 "exclude_nids": r.ExcludeNodeIDs} for r in j.Rules]}) for j in jobs]
    gd = [json.dumps({"id": k, "nids": g.NodeIDs}) for k, g in groups.items()]
    return jd, gd


def test_lock_units_kinds_and_contends():
    """The job index per rule (membership does not split a job), the jobs'
    Kind and AvgTime per rule from both job-set classes, and contends from the
    degrees of the host join model: the shadowed rule, the rule on no node and
    the paused job's rule reach no lock."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import join_model as JM
    from cronsun_amd import _lib
    from cronsun_amd.engine import contends_of
    from cronsun_amd.ingest import EtcdJobSet
    from cronsun_amd.model import JobSet, lock_units
    jobs, groups = _jobs()
    js = JobSet(jobs, groups)
    jd, gd = _docs()
    ejs = EtcdJobSet(jd, gd, threads=2)
    assert not ejs.job_status.any()
    for s in (js, ejs):
        rin = s.rules_in()
        unit = lock_units(rin)
        assert unit.dtype == np.int32 and unit.tolist() == [0, 0, 1, 1, 2, 2, 2, 3]
        kind, avg = s.rule_kinds()
        assert kind.dtype == np.int32 and kind.tolist() == [0, 0, 2, 2, 1, 1, 1, 1]
        assert avg.dtype == np.int64 and avg.tolist() == [40_000, 40_000, -7, -7, 2500, 2500, 2500, 0]
        for mode in (_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE):
            ct = contends_of(JM.join(rin, mode)[0])
            assert ct.dtype == np.uint8 and ct.tolist() == [1, 1, 1, 1, 0, 1, 0, 0], mode
    assert contends_of([0, 0, 3, 3, 4]).tolist() == [0, 1, 0, 1]
    bad = js.rules_in()
    bad.rule_job = np.array([0, 0, 2, 2, 1, 1, 1, 3], dtype=np.int32)
    with pytest.raises(ValueError, match="contiguous"):
        lock_units(bad)


def test_lock_profile_without_a_device_fails_loudly():
    """No CPU fallback: node_lock_skips / job_lock_runs need an MI355X.  Where
    one is visible: the 2500-ms alone job @every 60s runs every other minute,
    on whichever of n0 / n1 wins."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.model import JobSet
    jobs, groups = _jobs()
    js = JobSet(jobs[2:3], groups)
    t0 = 1767225600
    if engine.device_count() > 0:
        runs = js.job_lock_runs(t0, 60, 6)
        assert list(runs) == ["alone"]
        # rule c is on no node: its fires count as granted rows (it contends nowhere), rule b's alternate
        assert runs["alone"][1].tolist() == [0, 1, 0, 1, 0, 1]
        skips = js.node_lock_skips(t0, 60, 6)
        assert skips["n0"].tolist() == [0, 1, 0, 1, 0, 1] and skips["n1"].tolist() == [0, 1, 0, 1, 0, 1]
        return
    for call in (js.node_lock_skips, js.job_lock_runs):
        with pytest.raises(_lib.CgError) as e:
            call(t0, 60, 6)
        assert e.value.code == _lib.CG_ENODEV
