"""The admission profile entry points from plain C (tests/native/abi_admit_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on a ten-rule
set in six units, in the call order of the cgo stub's Admit / AdmitPerNode /
NodePeaks.  CPU: the program compiles, links and reports CG_ENODEV.  GPU: its
refusals hold (they are the program's exit code), and the matrices and peaks it
prints are compared with the literal model over the oracle's expansion and
Job.Cmds filter."""
import os
import subprocess

import numpy as np
import pytest

import admit_model as AM
import inflight_model as IM
import oracle_lib as O
from common import ZONEINFO, oracle_zone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_admit_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_admit_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
SPECS = ["0 */5 * * * *", "0 30 9 * * 1-5", "*/10 * * * * *", "*/15 * * * * *", "@every 90s", "0 0 0 30 Feb ?",
         "0 30 2 * * *", "7,30,45 * * * * *", "@every 7s", "* * * * * *"]
DUR = [400000, 400000, 25000, 25000, 180001, 0, 0, 20000, 20000, IM.INT64_MAX]
PAR = [1, 1, 2, 2, 1, 1, 1, 16, 16, 2]
UNIT = [0, 0, 3, 3, 4, 7, 7, 8, 8, 9]
W, B = 1800, 24
T0 = 1772953200 - 6 * 3600 + 17


@pytest.fixture(scope="module")
def abi_admit_c():
    lib = os.path.join(LIBDIR, "libcronsun_gpu.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(lib)):
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-o", BIN,
                               SRC, "-L" + LIBDIR, "-lcronsun_gpu", "-Wl,-rpath," + LIBDIR])
    return BIN


def _run(binary):
    out = subprocess.run([binary, ZONEINFO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = {}
    for ln in out.stdout.splitlines():
        k, _, rest = ln.partition(" ")
        lines.setdefault(k, []).append(rest)
    return lines


def test_header_is_c11_and_program_links(abi_admit_c):
    from cronsun_amd import engine
    lines = _run(abi_admit_c)
    assert lines["J"] == ["rules 10 nodes 5"]
    if engine.device_count() == 0:
        assert "NODEV" in lines


@pytest.mark.gpu
def test_admit_from_c_matches_model(abi_admit_c):
    from cronsun_amd.engine import RulesIn
    lines = _run(abi_admit_c)
    assert "OK" in lines
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    eo, et = O.expand_batch(O.sched_array(sch), T0, T0 + W * B, oracle_zone("America/New_York"))
    adm, drop = AM.admit_from_lists(eo, et, T0, W, B, DUR, PAR, UNIT)
    assert drop[0].any() and drop[4].any() and not drop[5:7].any() and not drop[7:9].any()
    assert int(adm[9].sum()) == 2 and int(drop[9].sum()) == W * B - 2  # runs past the horizon: two instances
    for key, tot, exp in (("D", "S", drop), ("A", "T", adm)):
        got = np.array([[int(x) for x in ln.split()] for ln in lines[key]])
        assert np.array_equal(got, exp), key
        assert [int(x) for x in lines[tot][0].split()] == exp.sum(axis=0).tolist()
    assert lines["K"] == ["3", "2", "3", "1"]
    # the C program's jobset, restated as integer arrays for the oracle: one job per unit
    groups = {"g1": ["n1", "n2", "n3"], "g2": ["n3", "n4"]}
    nodes = ["n1", "n2", "n3", "n4", "n5"]
    gl = [[nodes.index(n) for n in groups[g]] for g in ("g1", "g2")]
    job = np.unique(UNIT, return_inverse=True)[1]
    has_n5 = [int(u % 3 == 0) for u in UNIT]
    rin = RulesIn(len(nodes), 2, R, int(job.max()) + 1,
                  group_off=np.cumsum([0] + [len(x) for x in gl]), group_nodes=sum(gl, []),
                  group_exists=[1, 1], rule_job=job,
                  nid_off=np.cumsum([0] + has_n5), nids=[nodes.index("n5")] * sum(has_n5),
                  gid_off=np.arange(R + 1), gids=[0 if u % 2 else 1 for u in UNIT],
                  ex_off=np.zeros(R + 1, dtype=np.int64), ex=[], job_pause=[0] * (int(job.max()) + 1))
    roff, rules = O.node_rules(rin, 0, np.arange(len(nodes)))
    got_nodes = {ln.split(" ", 1)[0]: [int(x) for x in ln.split()[1:]] for ln in lines["M"]}
    got_peaks = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines["P"]}
    for k, name in enumerate(nodes):
        row = drop[rules[roff[k]:roff[k + 1]]].sum(axis=0, dtype=np.int64)
        assert got_nodes[name] == row.tolist(), name
        assert got_peaks[name] == [int(row.max()), int(row.argmax())], name
