"""The admission profile at the API surface (no compute here): the header
declares the two entry points, the two kinds and the ring limit and states the
definition; the ABI version stays 3; the built library exports the calls, _lib
binds them, the Python surface exists and refuses a bad `what` or a wrong
array shape before any device use; the job-set helpers give Parallels after
alone() and form units, splitting and reporting a job whose rules differ in
membership; the Go stub has the wrappers; README and DESIGN no longer list
Parallels as unmodelled.  Without a device the valid call is CG_ENODEV."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = {"cg_admit_device": 10, "cg_admit_per_node_device": 12}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_admit_entry_points():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"#define\s+CG_PROFILE_ADMITTED\s+2\b", txt)
    assert re.search(r"#define\s+CG_PROFILE_DROPPED\s+3\b", txt)
    assert re.search(r"#define\s+CG_ADMIT_MAX_PARALLELS\s+16\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    # dur_ms, parallels, unit, what -- then the rule set and mode in the per-node call
    args = r"n_buckets,\s*const\s+int64_t\s*\*\s*dur_ms\s*,\s*const\s+int64_t\s*\*\s*parallels\s*,\s*" \
           r"const\s+int32_t\s*\*\s*unit\s*,\s*int\s+what"
    assert re.search(r"cg_admit_device\s*\([^)]*" + args + r"\s*\)", txt)
    assert re.search(r"cg_admit_per_node_device\s*\([^)]*" + args +
                     r"\s*,\s*const\s+cg_rules\s*\*\s*rules,\s*int\s+mode\s*\)", txt)


def test_header_states_the_definition():
    raw = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    for phrase in ("does not decrease along r", "a contiguous rule range [u0, u1)", "the job's Count on one node",
                   "time ascending, rule index ascending", "fewer than P already admitted fires a",
                   "a*1000 + dur_ms > t*1000", "A fire at the very second an earlier instance ends is admitted",
                   "dur_ms == 0 admits everything", "admitted + dropped == the start profile",
                   "Commands started at or before t0 are unknown", "Here rule order decides",
                   "An alone job is limited per node only", "Actual run times differ from AvgTime",
                   "P >= k*d", "CG_ADMIT_MAX_PARALLELS"):
        assert phrase in raw, phrase


def test_docs_no_longer_list_parallels_as_unmodelled():
    for name in ("README.md", "DESIGN.md"):
        txt = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert not re.search(r"Parallels`? drops[^.]*(not modelled|not reproduced)", txt, flags=re.I), name
        assert "cg_admit_device" in txt and "KindInterval" in txt, name
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("k_admit_units", "admit_bench.json", "split"):
        assert phrase in design, phrase


def test_library_exports_admit_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_admit_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name, arity in NEW.items():
        assert name in _lib.SYMBOLS
        assert len(getattr(L, name).argtypes) == arity, name
    assert (_lib.PROFILE_ADMITTED, _lib.PROFILE_DROPPED, _lib.ADMIT_MAX_PARALLELS) == (2, 3, 16)


def test_python_surface():
    from cronsun_amd import engine, ingest, model
    for m in ("admit", "admit_per_node", "admit_device", "admit_kernel_times"):
        assert callable(getattr(engine.Engine, m))
    for cls in (model.JobSet, ingest.EtcdJobSet):
        assert callable(cls.node_drops) and callable(cls.rule_parallels)


def test_go_stub_has_the_wrappers():
    go = open(os.path.join(ROOT, "node", "cron", "gpu", "gpu.go")).read()
    assert re.search(r"func \(e \*Engine\) Admit\(", go)
    assert re.search(r"func \(e \*Engine\) AdmitPerNode\(", go)
    assert "ProfileAdmitted" in go and "ProfileDropped" in go


def test_python_refusals_need_no_device():
    """A bad `what` and arrays of the wrong length are refused by Engine.admit*
    before the library is called (no Engine is constructed here: the checks
    are the argument helper's)."""
    from cronsun_amd.engine import Engine
    e = Engine.__new__(Engine)  # no device behind it
    with pytest.raises(ValueError, match="what"):
        e._admit_args(2, [0, 0], [1, 1], None, "inflight")
    with pytest.raises(ValueError, match="dur_ms"):
        e._admit_args(2, [0], [1, 1], None, "dropped")
    with pytest.raises(ValueError, match="parallels"):
        e._admit_args(2, [0, 0], [1], None, "dropped")
    with pytest.raises(ValueError, match="unit"):
        e._admit_args(2, [0, 0], [1, 1], [0], "admitted")
    d, p, u, w = e._admit_args(2, [5, 5], [1, 1], [3, 3], "admitted")
    assert (d.dtype, p.dtype, u.dtype, w) == (np.int64, np.int64, np.int32, 2)
    assert e._admit_args(0, [], [], None, "dropped")[3] == 3


def test_null_handles_are_refused_before_any_device_use():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_admit_device(None, None, None, 0, 60, 4, None, None, None, 2) == _lib.CG_EINVAL
    assert L.cg_admit_per_node_device(None, None, None, 0, 60, 4, None, None, None, 3, None, 0) == _lib.CG_EINVAL


def _jobs():
    from cronsun_amd.model import Group, Job, JobRule, KindAlone
    g = {"g": Group("g", "", ["n0", "n1"]), "h": Group("h", "", ["n1", "n2"])}
    jobs = [
        # one unit: two rules with the same groups
        Job("same", Rules=[JobRule("a", "@every 30s", ["g"], [], []), JobRule("b", "@every 45s", ["g"], [], [])],
            Parallels=2, AvgTime=40_000),
        # differing GroupIDs: split
        Job("differs", Rules=[JobRule("a", "@every 30s", ["g"], [], []), JobRule("b", "@every 30s", ["h"], [], [])],
            Parallels=1, AvgTime=40_000),
        # alone: one instance whatever Parallels says; excludes differ (matter under an exclude mode only)
        Job("alone", Rules=[JobRule("a", "@every 10s", ["g"], ["n2"], []),
                            JobRule("b", "@every 10s", ["g"], ["n2"], ["n0"])],
            Parallels=7, Kind=KindAlone, AvgTime=15_000),
        Job("free", Rules=[JobRule("a", "* * * * * *", [], ["n0"], [])], Parallels=-3, AvgTime=0),
    ]
    return jobs, g


def _docs():
    jobs, groups = _jobs()
    jd = [json.dumps({"id": j.ID, "kind": j.Kind, "parallels": j.Parallels, "avg_time": j.AvgTime,
                      "rules": [{"id": r.ID, "timer": r.Timer, "gids": r.GroupIDs, "nids": r.NodeIDs,
                                 "exclude_nids": r.ExcludeNodeIDs} for r in j.Rules]}) for j in jobs]
    gd = [json.dumps({"id": k, "nids": g.NodeIDs}) for k, g in groups.items()]
    return jd, gd


def test_rule_parallels_and_unit_formation():
    """Parallels after alone() per rule; a job whose rules share their
    membership is one unit, one whose rules differ is split into one-rule
    units and reported; ExcludeNodeIDs count under an exclude mode only."""
    from cronsun_amd import _lib
    from cronsun_amd.ingest import EtcdJobSet
    from cronsun_amd.model import JobSet, admission_units
    jobs, groups = _jobs()
    js = JobSet(jobs, groups)
    jd, gd = _docs()
    ejs = EtcdJobSet(jd, gd, threads=2)
    assert not ejs.job_status.any()
    for s in (js, ejs):
        par = s.rule_parallels()
        assert par.dtype == np.int64 and par.tolist() == [2, 2, 1, 1, 1, 1, 0]
        unit, split = admission_units(s.rules_in(), _lib.EXCLUDE_NONE)
        assert unit.dtype == np.int32 and (np.diff(unit) >= 0).all()
        assert unit[0] == unit[1] and unit[2] != unit[3] and unit[4] == unit[5]
        assert len(set(unit.tolist())) == 5 and split == [1]
        for mode in (_lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE):
            unit, split = admission_units(s.rules_in(), mode)
            assert unit[0] == unit[1] and unit[2] != unit[3] and unit[4] != unit[5]
            assert len(set(unit.tolist())) == 6 and split == [1, 2] and (np.diff(unit) >= 0).all()


def test_node_drops_without_a_device_fails_loudly():
    """No CPU fallback: node_drops needs an MI355X.  Where one is visible: the
    alone job fires every 10 s twice over (two rules, one unit) and runs 15 s,
    so of each 10-s pair only every other lower-rule fire runs."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.model import JobSet
    jobs, groups = _jobs()
    js = JobSet(jobs[2:3], groups)
    t0 = 1767225600
    if engine.device_count() > 0:
        rows, split = js.node_drops(t0, 20, 3)
        # fires at +10 (a admitted, b dropped), +20 (both dropped: the run ends at +25), +30 (a admitted) ...
        assert split == [] and rows["n0"].tolist() == [3, 3, 3] and rows["n2"].tolist() == [3, 3, 3]
        adm, _ = js.node_drops(t0, 20, 3, what="admitted")
        assert adm["n1"].tolist() == [1, 1, 1]
        return
    with pytest.raises(_lib.CgError) as e:
        js.node_drops(t0, 20, 3)
    assert e.value.code == _lib.CG_ENODEV
