"""The fire-verdict entry points from plain C (tests/native/abi_verdict_c.c,
gcc -std=c11 -pedantic -Werror against include/cronsun_gpu.h) on a six-rule
set with both argument structs.  CPU: the program compiles, links and reports
CG_ENODEV.  GPU: its refusals hold (both structs NULL, the accessors before any
call and after a later expansion -- they are the program's exit code), and the
fires, bytes and selections it prints are compared with the literal model over
the oracle's expansion and lockTtl."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import verdict_model as VM
from common import ZONEINFO, oracle_zone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "abi_verdict_c.c")
BIN = os.path.join(ROOT, "tests", "native", "abi_verdict_c")
LIBDIR = os.path.join(ROOT, "cronsun_amd")
SPECS = ["*/10 * * * * *", "*/15 * * * * *", "@every 90s", "0 0 0 30 Feb ?", "0 * * * * *", "7,30,45 * * * * *"]
DUR = [25000, 25000, 180001, 0, 20000, 20000]
PAR = [2, 2, 1, 1, 1, 1]
UNIT = [0, 0, 3, 4, 7, 7]
KIND = [0, 0, 1, 1, 2, 2]
AVG = [25000, 25000, 180001, 180001, 20000, 20000]
JOB = [0, 0, 1, 1, 2, 2]
CONTENDS = [1, 1, 1, 1, 1, 0]
T0 = 1772953200 - 900 + 17
T1 = T0 + 1800


@pytest.fixture(scope="module")
def abi_verdict_c():
    lib = os.path.join(LIBDIR, "libcronsun_gpu.so")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(lib)):
        subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-o", BIN,
                               SRC, "-L" + LIBDIR, "-lcronsun_gpu", "-Wl,-rpath," + LIBDIR])
    return BIN


def _run(binary):
    out = subprocess.run([binary, ZONEINFO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def test_header_is_c11_and_program_links(abi_verdict_c):
    from cronsun_amd import engine
    lines = _run(abi_verdict_c)
    assert lines[0] == "J rules 6"
    if engine.device_count() == 0:
        assert lines[1].startswith("NODEV")


@pytest.mark.gpu
def test_verdicts_from_c_match_model(abi_verdict_c):
    lines = _run(abi_verdict_c)
    assert lines[-1] == "OK"
    R = len(SPECS)
    sch = [O.parse(s)[0] for s in SPECS]
    loc = oracle_zone("America/New_York")
    eo, et = O.expand_batch(O.sched_array(sch), T0, T1, loc)
    exp = VM.verdicts_from_lists(eo, et, T0, T1, admit=(DUR, PAR, UNIT), lock=(KIND, AVG, JOB, CONTENDS),
                                 ttl_of=lambda r, t: O.lock_ttl(sch[r], t, loc, KIND[r], AVG[r], 300))
    assert (exp & 1).any() and (exp & 2).any() and (exp == 3).any() and (exp == 0).any()
    assert not (exp[eo[0]:eo[2]] & 2).any() and not (exp[eo[5]:eo[6]] & 2).any()  # COMMON; a non-contending rule
    assert lines[1] == f"N {int(eo[R])}"
    rows = [ln for ln in lines if ln.startswith("V")]
    assert len(rows) == R
    for r, ln in enumerate(rows):
        got = [tuple(int(x) for x in tok.split(":")) for tok in ln.split()[1:]]
        want = list(zip(et[eo[r]:eo[r + 1]].tolist(), exp[eo[r]:eo[r + 1]].tolist()))
        assert got == want, f"rule {r}: first difference at fire " \
                            f"{next(i for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)}"
    at = [i for i, ln in enumerate(lines) if ln.startswith("S ")]
    assert len(at) == 3
    for i, (mask, value) in zip(at, ((1, 1), (2, 2), (3, 0))):
        so, st = VM.select(eo, et, exp, mask, value)
        assert lines[i] == f"S {mask} {value} {len(st)}"
        for r in range(R):
            got = [int(x) for x in lines[i + 1 + r].split()[1:]]
            assert got == st[so[r]:so[r + 1]].tolist(), (mask, value, r)
