"""The fire-verdict routine the kernels run (cg_verdict.h: fire_position over
the run records of count_rule and their prefix sum; the unit walks of
cg_admit.h / cg_lock.h with the emit that clears a bit there), compiled for the
host and checked byte by byte against the literal processes of the definition
run over the oracle's Next loop and or_lock_ttl (tests/native/verdict_host.cpp).
For every fire of every rule fire_position must be its index in the oracle's
rule-major list.  Zones, specs, t0 choices and shapes are
test_admit_algorithm.py's; units of 1, 2, 5 and 9 rules, P in {0, 1, 2, 16} with
its durations, test_lock_algorithm.py's kinds, AvgTimes and LockTtls.  The same
program also runs once under AddressSanitizer and UBSan: it is host code with
its own main.  CPU only: the GPU tests check the kernels themselves."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "verdict_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "verdict_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


def _build(out, extra):
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_verdict.h", "cg_lock.h", "cg_admit.h", "cg_profile.h",
                                                    "cg_expand.h", "cg_time.h", "cg_zone.h")]
    deps.append(os.path.join(ROOT, "tests", "native", "host_common.h"))
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-o", out] + extra + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def verdict_host():
    return _build(BIN, ["-O2"])


# zones whose 2026 transitions leave walked runs inside the checked horizons
WALKED = {"America/Havana", "Australia/Lord_Howe", "Pacific/Chatham"}


def _check(out, zone):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout
    # horizons the oracle reports as non-terminating are skipped and counted:
    # at most a quarter of a zone's may be
    line = [l for l in out.stdout.splitlines() if "horizons skipped" in l][0]
    print(line)
    skipped, n_all = int(line.split(": ")[1].split()[0]), int(line.split(" of ")[1].split()[0])
    assert n_all >= 8 and 4 * skipped <= n_all, line
    last = out.stdout.splitlines()[-1]
    print(last)

    def num(what):
        return int(re.search(r"(\d+) " + what, last).group(1))
    assert num("positions checked") > 0
    assert num("admission walks") > 0 and num("lock walks") > 0
    assert num("fires dropped") > 0 and num("fires skipped") > 0, last
    if zone in WALKED:
        assert num("of them in walked runs") > 0, last


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_verdicts_match_the_literal_processes(verdict_host, zone):
    out = subprocess.run([verdict_host, zone, "60", "11", "8000"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    _check(out, zone)


def test_host_verdicts_under_sanitizers():
    """The stand-alone program built with -fsanitize=address,undefined, on the
    zone with the most walked runs and a smaller fire budget."""
    binary = _build(BIN + "_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([binary, "Pacific/Chatham", "40", "11", "4000"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    _check(out, "Pacific/Chatham")
