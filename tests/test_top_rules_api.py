"""The top-rules calls at the API surface (no compute here): the header
declares the five entry points and CG_TOP_RULES_MAX, the ABI version stays 3,
the header comment carries the definition, the built library exports the
symbols, _lib binds them, and the Python surface exists."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = {"cg_profile_top_rules_nodes": 3, "cg_profile_top_rules_bucket": 3, "cg_profile_top_rules_copy": 8,
       "cg_profile_top_rules_device": 8, "cg_profile_top_rules_times": 3}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_top_rules_entry_points():
    txt = _header()
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
    assert re.search(r"#define\s+CG_TOP_RULES_MAX\s+64\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)
    assert re.search(r"cg_profile_top_rules_nodes\s*\(\s*cg_ctx\s*\*\s*ctx,\s*int32_t\s+k,\s*const\s+int32_t\s*\*\s*"
                     r"bucket\s*\)", txt)
    assert re.search(r"cg_profile_top_rules_bucket\s*\(\s*cg_ctx\s*\*\s*ctx,\s*int32_t\s+bucket,\s*int32_t\s+k\s*\)",
                     txt)


def test_header_states_the_definition():
    raw = " ".join(open(HEADER).read().split()).replace(" * ", " ")
    for phrase in ("count descending, rule index ascending", "never listed", "has been replaced"):
        assert phrase in raw, phrase


def test_library_exports_top_rules_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_top_rules_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name, arity in NEW.items():
        assert name in _lib.SYMBOLS
        assert len(getattr(L, name).argtypes) == arity, name
    assert _lib.TOP_RULES_MAX == 64


def test_python_surface():
    from cronsun_amd import engine, ingest, model
    for m in ("profile_top_rules", "profile_top_rules_bucket", "profile_top_rules_device", "profile_top_rules_ms",
              "profile_top_rules_copy"):
        assert callable(getattr(engine.Engine, m))
    for cls in (model.JobSet, ingest.EtcdJobSet):
        assert callable(cls.node_peak_rules)


def test_go_stub_has_the_wrappers():
    go = open(os.path.join(ROOT, "node", "cron", "gpu", "gpu.go")).read()
    assert re.search(r"func \(e \*Engine\) TopRules\(j \*Jobset, k int\)", go)
    assert re.search(r"func \(e \*Engine\) TopRulesBucket\(bucket, k int\)", go)


def test_node_peak_rules_without_a_device_fails_loudly():
    """No CPU fallback: node_peak_rules needs an MI355X (where one is visible
    it works: the rule every 10 s leads the one every 30 s in a minute)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    js = JobSet([Job("j0", Rules=[JobRule("r0", "@every 30s", ["g"], [], [])]),
                 Job("j1", Rules=[JobRule("r0", "@every 10s", ["g"], [], [])])], {"g": Group("g", "", ["n0"])})
    t0 = 1767225600
    if engine.device_count() > 0:
        assert js.node_peak_rules(t0, 60, 4, k=2) == {"n0": (8, 0, [("j1", "r0", 6), ("j0", "r0", 2)])}
        return
    with pytest.raises(_lib.CgError) as e:
        js.node_peak_rules(t0, 60, 4)
    assert e.value.code == _lib.CG_ENODEV
