"""The dispatcher's node fan-out at the API surface (no compute here): the
header declares the entry points, the built library exports them, _lib binds
them, the ABI version stays 3, and ClusterCron fails loudly without a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = ["cg_dispatcher_bind_rules", "cg_dispatcher_fanout", "cg_dispatcher_fanout_copy",
       "cg_dispatcher_fanout_range", "cg_dispatcher_fanout_device", "cg_dispatcher_set_fanout_path"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_fanout_entry_points():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    for name, val in (("CG_FANOUT_AUTO", 0), ("CG_FANOUT_FILTER", 1), ("CG_FANOUT_DUE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)


def test_library_exports_fanout_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_fanout_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert (_lib.CG_FANOUT_AUTO, _lib.CG_FANOUT_FILTER, _lib.CG_FANOUT_DUE) == (0, 1, 2)


def test_python_surface():
    from cronsun_amd import dispatch, engine
    for m in ("bind_rules", "fanout", "fanout_range", "set_fanout_path"):
        assert callable(getattr(engine.Dispatcher, m))
    assert callable(engine.Engine.fanout_ms)
    assert callable(dispatch.ClusterCron)


def test_cluster_cron_without_a_device_fails_loudly():
    """No CPU fallback: begin() needs an MI355X (where one is visible it works)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.dispatch import ClusterCron
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    js = JobSet([Job("j0", Rules=[JobRule("r0", "@every 5s", ["g"], ["n1"], [])])],
                {"g": Group("g", "", ["n0"])})
    cc = ClusterCron(js)
    t0 = 1767225600
    if engine.device_count() > 0:
        cc.begin(t0)
        assert cc.effective == t0 + 5
        cc.close()
        return
    with pytest.raises(_lib.CgError) as e:
        cc.begin(t0)
    assert e.value.code == _lib.CG_ENODEV
