"""cg_dispatcher_upcoming* at the API surface (no compute here): the header
declares the entry points and CG_UPCOMING_MAX, the built library exports them,
_lib binds them, the ABI version stays 3, the Python surface exists, and
ClusterCron.upcoming fails loudly without a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")

NEW = ["cg_dispatcher_upcoming", "cg_dispatcher_upcoming_node", "cg_dispatcher_upcoming_copy",
       "cg_dispatcher_upcoming_device", "cg_dispatcher_upcoming_times"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_upcoming_entry_points():
    txt = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"#define\s+CG_UPCOMING_MAX\s+65536\b", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)


def test_library_exports_upcoming_entry_points():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (cg_[a-z0-9_]+)", out))
    assert not [n for n in NEW if n not in exported]


def test_lib_binds_upcoming_entry_points():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert _lib.UPCOMING_MAX == 65536


def test_python_surface():
    from cronsun_amd import dispatch, engine
    for m in ("upcoming", "upcoming_count", "upcoming_copy", "upcoming_device", "upcoming_ms"):
        assert callable(getattr(engine.Dispatcher, m))
    assert callable(dispatch.Cron.Upcoming)
    assert callable(dispatch.ClusterCron.upcoming)


def test_cron_upcoming_before_start_is_the_host_order():
    """Not running: nothing is in HBM, Next is what Stop left (zero before the
    first Start), and no entry is firing."""
    from cronsun_amd.dispatch import Cron, Entry
    c = Cron()
    c.AddFunc("* * * * * ?", lambda: None)
    assert c.Upcoming(5) == []
    e = c._entries[0]
    c._entries[0] = Entry(ID=e.ID, Schedule=e.Schedule, Next=100, Prev=90, Job=e.Job)
    got = c.Upcoming(5)
    assert [(x.Next, x.Prev) for x in got] == [(100, 90)] and c.Upcoming(5, until=99) == []
    with pytest.raises(ValueError):
        c.Upcoming(0)


def test_cluster_cron_upcoming_without_a_device_fails_loudly():
    """No CPU fallback: upcoming() needs an MI355X (where one is visible it works)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.dispatch import ClusterCron
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    js = JobSet([Job("j0", Rules=[JobRule("r0", "@every 5s", ["g"], ["n1"], [])])],
                {"g": Group("g", "", ["n0"])})
    cc = ClusterCron(js)
    t0 = 1767225600
    if engine.device_count() > 0:
        cc.begin(t0)
        assert cc.upcoming(3) == [(t0 + 5, ("j0", "r0"))]
        assert cc.upcoming(3, node_id="n0") == [(t0 + 5, ("j0", "r0"))]
        with pytest.raises(KeyError):
            cc.upcoming(3, node_id="nowhere")
        cc.close()
        return
    with pytest.raises(_lib.CgError) as e:
        cc.upcoming(3)
    assert e.value.code == _lib.CG_ENODEV
