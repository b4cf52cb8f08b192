"""The in-flight profile entry points from plain C (tests/native/abi_inflight_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on a ten-rule
set, in the call order of the cgo stub's InFlight / InFlightPerNode /
NodePeaks.  CPU: the program compiles, links and reports CG_ENODEV.  GPU: the
matrices and peaks it prints are compared with the model over the oracle's
expansion and Job.Cmds filter."""
import os
import subprocess

import numpy as np
import pytest

import inflight_model as IM
import oracle_lib as O
from common import ZONEINFO, oracle_zone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_inflight_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_inflight_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
SPECS = ["0 */5 * * * *", "0 30 9 * * 1-5", "*/10 * * * * *", "@daily", "@every 90s", "0 0 0 30 Feb ?",
         "0 30 2 * * *", "@hourly", "7,30,45 * * * * *", "@every 7s"]
DUR = [0, 300, 1799999, 1800000, 1800001, 7200000, 18000000, 1001, IM.INT64_MAX, 60000]
W, B = 1800, 24
T0 = 1772953200 - 6 * 3600 + 17


@pytest.fixture(scope="module")
def abi_inflight_c():
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


def test_header_is_c11_and_program_links(abi_inflight_c):
    from cronsun_amd import engine
    lines = _run(abi_inflight_c)
    assert lines["J"] == ["rules 10 nodes 5"]
    if engine.device_count() == 0:
        assert "NODEV" in lines


@pytest.mark.gpu
def test_inflight_from_c_matches_model(abi_inflight_c):
    from cronsun_amd.engine import RulesIn
    lines = _run(abi_inflight_c)
    assert "OK" in lines
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    eo, et = O.expand_batch(O.sched_array(sch), T0, T0 + W * B, oracle_zone("America/New_York"))
    exp = IM.inflight_from_lists(eo, et, T0, W, B, IM.seconds(DUR))
    starts = np.bincount(np.repeat(np.arange(R, dtype=np.int64), np.diff(eo)) * B + (et - T0 - 1) // W,
                         minlength=R * B).reshape(R, B)
    assert not exp[0].any() and np.array_equal(exp[3], starts[3])  # 0 ms; exactly one width
    assert np.array_equal(exp[8], np.cumsum(starts[8]))            # INT64_MAX ms: the prefix sums
    got = np.array([[int(x) for x in ln.split()] for ln in lines["R"]])
    assert np.array_equal(got, exp)
    assert [int(x) for x in lines["S"][0].split()] == exp.sum(axis=0).tolist()
    assert lines["K"] == ["1", "1", "0"]
    # the C program's jobset, restated as integer arrays for the oracle
    groups = {"g1": ["n1", "n2", "n3"], "g2": ["n3", "n4"]}
    nodes = ["n1", "n2", "n3", "n4", "n5"]
    gl = [[nodes.index(n) for n in groups[g]] for g in ("g1", "g2")]
    rin = RulesIn(len(nodes), 2, R, R,
                  group_off=np.cumsum([0] + [len(x) for x in gl]), group_nodes=sum(gl, []),
                  group_exists=[1, 1], rule_job=np.arange(R),
                  nid_off=np.cumsum([0] + [int(i % 3 == 0) for i in range(R)]),
                  nids=[nodes.index("n5")] * sum(int(i % 3 == 0) for i in range(R)),
                  gid_off=np.arange(R + 1), gids=[0 if i % 2 else 1 for i in range(R)],
                  ex_off=np.cumsum([0] + [int(i % 4 == 0) for i in range(R)]),
                  ex=[nodes.index("n3")] * sum(int(i % 4 == 0) for i in range(R)),
                  job_pause=[int(i == 7) for i in range(R)])
    roff, rules = O.node_rules(rin, 0, np.arange(len(nodes)))
    got_nodes = {ln.split(" ", 1)[0]: [int(x) for x in ln.split()[1:]] for ln in lines["M"]}
    got_peaks = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines["P"]}
    start_rows = []
    for k, name in enumerate(nodes):
        row = exp[rules[roff[k]:roff[k + 1]]].sum(axis=0, dtype=np.int64)
        assert got_nodes[name] == row.tolist(), name
        assert got_peaks[name] == [int(row.max()), int(row.argmax())], name
        start_rows.append(starts[rules[roff[k]:roff[k + 1]]].sum(axis=0, dtype=np.int64))
    # the peaks of nodes 1 and 2 of the start profile that replaced it
    q = [int(x) for x in lines["Q"][0].split()]
    assert q == [int(start_rows[1].max()), int(start_rows[1].argmax()), int(start_rows[2].max()),
                 int(start_rows[2].argmax())]
