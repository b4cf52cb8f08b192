"""The running profile kinds from plain C (tests/native/abi_running_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on
abi_admit_c.c's ten-rule set.  CPU: the program compiles, links and reports
CG_ENODEV.  GPU: its refusals and kernel-time slots hold (they are the
program's exit code), and the matrices and peaks it prints are compared with
the literal model over the oracle's expansion, lockTtl and Job.Cmds filter."""
import os
import subprocess

import numpy as np
import pytest

import inflight_model as IM
import oracle_lib as O
import running_model as RM
from common import ZONEINFO, oracle_zone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_running_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_running_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
SPECS = ["0 */5 * * * *", "0 30 9 * * 1-5", "*/10 * * * * *", "*/15 * * * * *", "@every 90s", "0 0 0 30 Feb ?",
         "0 30 2 * * *", "7,30,45 * * * * *", "@every 7s", "* * * * * *"]
DUR = [400000, 400000, 25000, 25000, 1800000, 0, 0, 20000, 20000, IM.INT64_MAX]
PAR = [1, 1, 2, 2, 1, 1, 1, 16, 16, 2]
UNIT = [0, 0, 3, 3, 4, 7, 7, 8, 8, 9]
KIND = [1, 1, 2, 2, 0, 2, 2, 1, 1, 1]
CONTENDS = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
W, B, LOCK_TTL = 1800, 24, 300
T0 = 1772953200 - 6 * 3600 + 17


@pytest.fixture(scope="module")
def abi_running_c():
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


def test_header_is_c11_and_program_links(abi_running_c):
    from cronsun_amd import engine
    lines = _run(abi_running_c)
    assert lines["J"] == ["rules 10 nodes 5"]
    if engine.device_count() == 0:
        assert "NODEV" in lines


@pytest.mark.gpu
def test_running_from_c_matches_model(abi_running_c):
    from cronsun_amd.engine import RulesIn
    lines = _run(abi_running_c)
    assert "OK" in lines and lines["K"] == ["7", "8", "7", "2"]
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    loc = oracle_zone("America/New_York")
    eo, et = O.expand_batch(O.sched_array(sch), T0, T0 + W * B, loc)
    run, adm = RM.admit_running(eo, et, T0, W, B, DUR, PAR, UNIT)
    infl = IM.inflight_from_lists(eo, et, T0, W, B, np.minimum(IM.seconds(DUR), W * B))
    assert (run <= infl).all() and (run[0] < infl[0]).any() and np.array_equal(run[4], adm[4])  # d == w
    assert run[9].tolist() == [2] * B  # runs past the horizon: the two instances that ever start

    def ttl_of(r, t):
        return O.lock_ttl(sch[r], t, loc, KIND[r], DUR[r], LOCK_TTL)
    lrun, granted = RM.lock_running(eo, et, T0, W, B, KIND, DUR, UNIT, CONTENDS, ttl_of)
    assert np.array_equal(lrun[3], infl[3]) and np.array_equal(lrun[4], infl[4])  # non-contending, COMMON
    assert lrun[9].tolist() == [1] * B and (lrun[8] < infl[8]).any()
    for key, tot, exp in (("R", "T", run), ("L", "U", lrun)):
        got = np.array([[int(x) for x in ln.split()] for ln in lines[key]])
        assert np.array_equal(got, exp), key
        assert [int(x) for x in lines[tot][0].split()] == exp.sum(axis=0).tolist()
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
        row = run[rules[roff[k]:roff[k + 1]]].sum(axis=0, dtype=np.int64)
        assert got_nodes[name] == row.tolist(), name
        assert got_peaks[name] == [int(row.max()), int(row.argmax())], name
