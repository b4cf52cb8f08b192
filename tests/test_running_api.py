"""Running profile: the API surface that needs no device.  The header defines
the two kinds as 7 and 8 (6 stays unassigned) and states the definition; _lib
carries them; Engine.admit* / lock_runs* convert what="running" and keep
refusing the other flavour's words; without a device the new kinds end as kinds
2/3 and 4/5 do; JobSet / EtcdJobSet have node_running and job_lock_running and
node_peak_rules takes running=True; the Go stub has the constants; the docs
name the kinds and their limits."""
import os
import re

import numpy as np
import pytest

import test_admit_api as TA
import test_lock_profile_api as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")


def test_header_defines_the_kinds():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+CG_PROFILE_RUNNING\s+7\b", txt)
    assert re.search(r"#define\s+CG_PROFILE_LOCK_RUNNING\s+8\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    values = [int(v) for v in re.findall(r"#define\s+CG_PROFILE_[A-Z_]+\s+(\d+)\b", txt)]
    assert sorted(values) == [0, 1, 2, 3, 4, 5, 7, 8]  # 6 is not assigned


def test_header_states_the_definition():
    raw = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    for phrase in ("running[r][b] = #{ admitted fires a of rule r : e_b - d_r < a <= e_b }",
                   "running[r][b] = #{ granted fires g of rule r : e_b - d_r < g <= e_b }",
                   "Rows of units that never drop are the rows of cg_inflight_device",
                   "an INTERVAL command runs d_r seconds whatever its lease does",
                   "running <= in flight cell by cell", "sum to at most P at every edge",
                   "sum to at most 1 at every edge", "limit() and lock() are not composed",
                   "avg <= 0: a zero row", "the totals count each cluster-wide run once",
                   "`what` not 4, 5 or 8", "(k_rows_prefix)", "23 entries in all"):
        assert phrase in raw, phrase


def test_lib_constants_and_python_surface():
    from cronsun_amd import _lib, engine, ingest, model
    assert (_lib.PROFILE_RUNNING, _lib.PROFILE_LOCK_RUNNING) == (7, 8)
    assert callable(engine.Engine.running_kernel_times)
    assert "PROFILE_RUNNING" in engine.Engine.profile_kind.__doc__
    assert "PROFILE_LOCK_RUNNING" in engine.Engine.profile_kind.__doc__
    for cls in (model.JobSet, ingest.EtcdJobSet):
        assert callable(cls.node_running) and callable(cls.job_lock_running)
        assert "running" in cls.node_peak_rules.__code__.co_varnames
    assert callable(model.job_lock_running_of)


def test_what_running_is_converted_and_the_other_words_still_refused():
    from cronsun_amd.engine import Engine
    e = Engine.__new__(Engine)  # no device behind it
    d, p, u, w = e._admit_args(2, [5, 5], [1, 1], [3, 3], "running")
    assert (d.dtype, p.dtype, u.dtype, w) == (np.int64, np.int64, np.int32, 7)
    assert e._admit_args(0, [], [], None, "running")[3] == 7
    k, a, u, c, ttl, w = e._lock_args(2, [1, 2], [-5, 2500], [3, 4], [True, 7], 2, "running")
    assert (k.dtype, a.dtype, u.dtype, c.dtype, ttl, w) == (np.int32, np.int64, np.int32, np.uint8, 2, 8)
    assert e._lock_args(0, [], [], None, None, 300, "running")[5] == 8
    for word in ("inflight", "granted", "skipped", "lock_running", 7):
        with pytest.raises(ValueError, match="what"):
            e._admit_args(2, [0, 0], [1, 1], None, word)
    for word in ("dropped", "admitted", "inflight", 8):
        with pytest.raises(ValueError, match="what"):
            e._lock_args(2, [1, 1], [0, 0], None, None, 300, word)
    # the other argument checks apply to the new word as to the old ones
    with pytest.raises(ValueError, match="parallels"):
        e._admit_args(2, [0, 0], [1], None, "running")
    with pytest.raises(ValueError, match="lock_ttl"):
        e._lock_args(2, [1, 1], [0, 0], None, None, 1, "running")


def test_the_new_kinds_end_as_the_old_ones_without_a_handle():
    """Null handles: the argument check that precedes any device use answers
    kind 7 as it answers 2 and 3, and kind 8 as 4 and 5."""
    from cronsun_amd import _lib
    L = _lib.lib()
    adm = {w: L.cg_admit_device(None, None, None, 0, 60, 4, None, None, None, w) for w in (2, 3, 7)}
    assert set(adm.values()) == {_lib.CG_EINVAL}
    adm = {w: L.cg_admit_per_node_device(None, None, None, 0, 60, 4, None, None, None, w, None, 0) for w in (2, 3, 7)}
    assert set(adm.values()) == {_lib.CG_EINVAL}
    lk = {w: L.cg_lock_profile_device(None, None, None, 0, 60, 4, None, None, None, None, 300, w) for w in (4, 5, 8)}
    assert set(lk.values()) == {_lib.CG_EINVAL}
    lk = {w: L.cg_lock_profile_per_node_device(None, None, None, 0, 60, 4, None, None, None, None, 300, w, None, 0)
          for w in (4, 5, 8)}
    assert set(lk.values()) == {_lib.CG_EINVAL}


def test_node_running_plumbing():
    """No CPU fallback: without an MI355X node_running ends as node_drops does
    (CG_ENODEV).  Where one is visible: the alone job of test_admit_api fires
    every 10 s twice over and runs 15 s; the lower rule's fires at +10, +30
    and +50 start, and each still runs at the next 20-s edge."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.model import JobSet
    jobs, groups = TA._jobs()
    js = JobSet(jobs[2:3], groups)
    t0 = 1767225600
    if engine.device_count() > 0:
        rows, split = js.node_running(t0, 20, 3)
        assert split == [] and set(rows) == {"n0", "n1", "n2"}
        for n in rows:
            assert rows[n].dtype == np.int64 and rows[n].tolist() == [1, 1, 1], n
        infl, _ = js.node_inflight(t0, 20, 3)
        assert infl["n0"].tolist() == [4, 4, 4]  # every fire counted: +10 and +20 of both rules at the edge +20
        peaks, split = js.node_peak_rules(t0, 20, 3, k=4, running=True)
        assert split == [] and peaks["n0"] == (1, 0, [("alone", "a", 1)])
        with pytest.raises(ValueError):
            js.node_peak_rules(t0, 20, 3, inflight=True, running=True)
        return
    for call in (js.node_running, js.node_drops):
        with pytest.raises(_lib.CgError) as e:
            call(t0, 20, 3)
        assert e.value.code == _lib.CG_ENODEV


def test_job_lock_running_plumbing():
    """Without a device as job_lock_runs (CG_ENODEV).  With one: the 2500-ms
    alone job @every 60s of test_lock_profile_api runs every other minute
    (rule b, started at the 60-s edge itself: 1, 0, 1, ...); its rule a is
    replaced everywhere and its rule c is on no node, so neither reaches the
    lock and their rows are the in-flight rows (1 at every edge each)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.ingest import EtcdJobSet
    from cronsun_amd.model import JobSet
    jobs, groups = TL._jobs()
    js = JobSet(jobs[2:3], groups)
    t0 = 1767225600
    if engine.device_count() > 0:
        jd, gd = TL._docs()
        for s in (js, EtcdJobSet(jd[2:3], gd, threads=1)):
            run = s.job_lock_running(t0, 60, 6)
            assert list(run) == ["alone"] and run["alone"].dtype == np.int64
            assert run["alone"].tolist() == [3, 2, 3, 2, 3, 2]
        granted = js.job_lock_runs(t0, 60, 6)["alone"][0]
        assert granted.tolist() == [3, 2, 3, 2, 3, 2]  # d (3 s) <= w: every run is over by the next edge
        return
    for call in (js.job_lock_running, js.job_lock_runs):
        with pytest.raises(_lib.CgError) as e:
            call(t0, 60, 6)
        assert e.value.code == _lib.CG_ENODEV


def test_go_stub_has_the_constants():
    go = open(os.path.join(ROOT, "node", "cron", "gpu", "gpu.go")).read()
    assert re.search(r"ProfileRunning\s*=\s*C\.CG_PROFILE_RUNNING\b", go)
    assert re.search(r"ProfileLockRunning\s*=\s*C\.CG_PROFILE_LOCK_RUNNING\b", go)


def test_docs_name_the_kinds_and_their_limits():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        txt = " ".join(open(os.path.join(ROOT, name)).read().split())
        for phrase in ("CG_PROFILE_RUNNING", "CG_PROFILE_LOCK_RUNNING", "node_running", "job_lock_running"):
            assert phrase in txt, (name, phrase)
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("k_rows_prefix", "running_emit_diff", "running profile", "running_bench.json", "not composed",
                   "cold start"):
        assert phrase in design, phrase
