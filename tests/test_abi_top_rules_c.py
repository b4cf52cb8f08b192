"""The top-rules entry points from plain C (tests/native/abi_top_rules_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on the ten-rule,
five-node set of abi_inflight_c.c, in the call order of the cgo stub's
TopRules / TopRulesBucket.  CPU: the program compiles, links and reports
CG_ENODEV.  GPU: the lists it prints equal the model (top_rules_model.py) over
the in-flight model's rule matrix and the oracle's Job.Cmds filter."""
import os
import subprocess

import numpy as np
import pytest

import inflight_model as IM
import oracle_lib as O
import top_rules_model as TM
from common import ZONEINFO, oracle_zone
from test_abi_inflight_c import B, DUR, SPECS, T0, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_top_rules_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_top_rules_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
K = 3


@pytest.fixture(scope="module")
def abi_top_rules_c():
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


def test_header_is_c11_and_program_links(abi_top_rules_c):
    from cronsun_amd import engine
    lines = _run(abi_top_rules_c)
    assert lines["J"] == ["rules 10 nodes 5"]
    if engine.device_count() == 0:
        assert "NODEV" in lines


def _rows(lines, k):
    """The program's 'row bucket n_contrib n_listed rule:count ...' lines as
    the model's five arrays."""
    rule, count, nl, nc, bk = [], [], [], [], []
    for i, ln in enumerate(lines):
        f = ln.split()
        assert int(f[0]) == i and len(f) == 4 + k
        bk.append(int(f[1]))
        nc.append(int(f[2]))
        nl.append(int(f[3]))
        rule.append([int(x.split(":")[0]) for x in f[4:]])
        count.append([int(x.split(":")[1]) for x in f[4:]])
    i32 = lambda x, shape: np.array(x, dtype=np.int32).reshape(shape)  # noqa: E731
    n = len(lines)
    return i32(rule, (n, k)), i32(count, (n, k)), i32(nl, n), i32(nc, n), i32(bk, n)


@pytest.mark.gpu
def test_top_rules_from_c_match_model(abi_top_rules_c):
    from cronsun_amd.engine import RulesIn
    lines = _run(abi_top_rules_c)
    assert "OK" in lines
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    eo, et = O.expand_batch(O.sched_array(sch), T0, T0 + W * B, oracle_zone("America/New_York"))
    matrix = IM.inflight_from_lists(eo, et, T0, W, B, IM.seconds(DUR))
    # the C program's jobset, restated as integer arrays for the oracle (as test_abi_inflight_c.py)
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
    N = len(nodes)
    roff, rules = O.node_rules(rin, 0, np.arange(N))
    node_matrix = np.array([matrix[rules[roff[n]:roff[n + 1]]].sum(axis=0, dtype=np.int64) for n in range(N)])
    peak_at = IM.peaks(node_matrix)[1]
    exp = TM.top_rules(matrix, roff, rules, peak_at, K)
    assert (exp[3] > K).any() and (exp[3] < K).any()  # a cut list and a padded one
    TM.same("peak buckets", _rows(lines["P"], K), exp)
    assert lines["Q"] == lines["P"]  # the refused calls left the result readable
    TM.same("explicit buckets", _rows(lines["B"], K), TM.top_rules(matrix, roff, rules,
                                                                   [(5 * n + 3) % B for n in range(N)], K))
    assert lines["T"] == [str(N)]
    off1, all_rules = TM.cluster_lists(R)
    TM.same("cluster-wide, last bucket", _rows(lines["C"], 64), TM.top_rules(matrix, off1, all_rules, [B - 1], 64))
    TM.same("cluster-wide, bucket 0", _rows(lines["D"], 2), TM.top_rules(matrix, off1, all_rules, [0], 2))
