"""The fire-profile entry points from plain C (tests/native/abi_profile_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on a ten-rule
set, in the call order of the cgo stub's Profile / ProfilePerNode.  CPU: the
program compiles, links and reports CG_ENODEV.  GPU: the matrices it prints
are compared with the oracle's binned expansion and Job.Cmds filter."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from common import ZONEINFO, oracle_zone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_profile_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_profile_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
SPECS = ["0 */5 * * * *", "0 30 9 * * 1-5", "*/10 * * * * *", "@daily", "@every 90s", "0 0 0 30 Feb ?",
         "0 30 2 * * *", "@hourly", "7,30,45 * * * * *", "@every 7s"]
W, B = 1800, 24
T0 = 1772953200 - 6 * 3600 + 17


@pytest.fixture(scope="module")
def abi_profile_c():
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


def test_header_is_c11_and_program_links(abi_profile_c):
    from cronsun_amd import engine
    lines = _run(abi_profile_c)
    assert lines["J"] == ["rules 10 nodes 5"]
    if engine.device_count() == 0:
        assert "NODEV" in lines


@pytest.mark.gpu
def test_profile_from_c_matches_oracle(abi_profile_c):
    from cronsun_amd.engine import RulesIn
    lines = _run(abi_profile_c)
    assert "OK" in lines
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    eo, et = O.expand_batch(O.sched_array(sch), T0, T0 + W * B, oracle_zone("America/New_York"))
    rule = np.repeat(np.arange(R, dtype=np.int64), np.diff(eo))
    exp = np.bincount(rule * B + (et - T0 - 1) // W, minlength=R * B).reshape(R, B)
    got = np.array([[int(x) for x in ln.split()] for ln in lines["R"]])
    assert np.array_equal(got, exp)
    assert [int(x) for x in lines["S"][0].split()] == exp.sum(axis=0).tolist()
    assert [int(x) for x in lines["X"][0].split()] == exp[2].tolist()
    # no node matrix after cg_profile_device, one after the per-node call
    assert lines["D"] == [f"{R} 0 {B} rules 1 totals 1 nodes 0", f"{R} 5 {B} rules 1 totals 1 nodes 1"]
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
    for k, name in enumerate(nodes):
        assert got_nodes[name] == exp[rules[roff[k]:roff[k + 1]]].sum(axis=0).tolist(), name
