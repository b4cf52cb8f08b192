"""The in-flight profile at the API surface (no compute here): the header
declares the four entry points and the two kind constants, the ABI version
stays 3, the built library exports them, _lib binds them, the Python surface
exists, and the job-set helpers map AvgTime <= 0 to "no estimate" and count
those rules."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = ["cg_inflight_device", "cg_inflight_per_node_device", "cg_profile_kind", "cg_profile_node_peaks"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_inflight_entry_points():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"#define\s+CG_PROFILE_STARTS\s+0\b", txt)
    assert re.search(r"#define\s+CG_PROFILE_INFLIGHT\s+1\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    # dur_ms sits before the rule set in the per-node call
    assert re.search(r"cg_inflight_per_node_device\s*\([^)]*n_buckets,\s*const\s+int64_t\s*\*\s*dur_ms[^)]*"
                     r"const\s+cg_rules\s*\*\s*rules,\s*int\s+mode\s*\)", txt)


def test_header_states_the_definition():
    """The definition lives in the header comment: rounding up, the fires not
    counted, and what is not reproduced."""
    raw = " ".join(open(HEADER).read().split())
    for phrase in ("rounded UP", "e_b - d_r < t <= e_b", "started at or before t0", "Not reproduced",
                   "Job.Parallels", "KindAlone"):
        assert phrase in raw.replace(" * ", " "), phrase


def test_library_exports_inflight_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_inflight_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert len(L.cg_inflight_device.argtypes) == 7 and len(L.cg_inflight_per_node_device.argtypes) == 9
    assert (_lib.PROFILE_STARTS, _lib.PROFILE_INFLIGHT) == (0, 1)


def test_python_surface():
    from cronsun_amd import engine, ingest, model
    for m in ("inflight", "inflight_per_node", "inflight_device", "inflight_per_node_device", "profile_kind",
              "profile_node_peaks"):
        assert callable(getattr(engine.Engine, m))
    for cls in (model.JobSet, ingest.EtcdJobSet):
        assert callable(cls.node_inflight) and callable(cls.rule_durations)


def test_jobset_durations_map_no_estimate_to_zero():
    """Each rule takes its job's AvgTime; AvgTime <= 0 (never run, or the
    reference's negative values) counts as 0 and is reported."""
    from cronsun_amd.ingest import EtcdJobSet
    from cronsun_amd.model import Group, Job, JobRule, JobSet, durations_of
    avgs = [4200, 0, -7, 1, 7_200_000]
    jobs = [Job(f"j{i}", Rules=[JobRule(f"r{k}", "@every 30s", ["g"], [], []) for k in range(1 + i % 2)], AvgTime=a)
            for i, a in enumerate(avgs)]
    js = JobSet(jobs, {"g": Group("g", "", ["n0", "n1"])})
    dur, missing = js.rule_durations()
    assert dur.dtype == np.int64 and dur.tolist() == [4200, 0, 0, 0, 1, 1, 7_200_000]
    assert missing == 3
    docs = [json.dumps({"id": f"j{i}", "avg_time": a,
                        "rules": [{"id": f"r{k}", "timer": "@every 30s", "gids": ["g"]} for k in range(1 + i % 2)]})
            for i, a in enumerate(avgs)]
    ejs = EtcdJobSet(docs, [json.dumps({"id": "g", "nids": ["n0", "n1"]})], threads=2)
    assert not ejs.job_status.any()
    dur2, missing2 = ejs.rule_durations()
    assert dur2.tolist() == dur.tolist() and missing2 == 3
    d, n = durations_of([])
    assert d.shape == (0,) and n == 0


def test_node_inflight_without_a_device_fails_loudly():
    """No CPU fallback: node_inflight needs an MI355X (where one is visible it
    works: one rule every 30 s running 45 s is twice in flight at every edge
    but the first)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    js = JobSet([Job("j0", Rules=[JobRule("r0", "@every 30s", ["g"], [], [])], AvgTime=45_000),
                 Job("j1", Rules=[JobRule("r0", "@every 30s", ["g"], [], [])])], {"g": Group("g", "", ["n0"])})
    t0 = 1767225600
    if engine.device_count() > 0:
        rows, missing = js.node_inflight(t0, 30, 4)
        assert missing == 1 and rows["n0"].tolist() == [1, 2, 2, 2]
        return
    with pytest.raises(_lib.CgError) as e:
        js.node_inflight(t0, 30, 4)
    assert e.value.code == _lib.CG_ENODEV
