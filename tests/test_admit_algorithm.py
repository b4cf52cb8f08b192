"""The admission routine the kernel runs (cg_admit.h: admit_walk_unit over the
run records of count_rule, with its closed forms, walked runs and skips),
compiled for the host and checked cell by cell, in both kinds, against the
literal process of the definition run over the oracle's Next loop
(tests/native/admit_host.cpp).  Zones, specs, t0 choices and shapes are
test_profile_algorithm.py's; the rules of a horizon form units of 1, 2, 5 and
9 (one more than the remembered walked-run positions),
each checked with P in {0, 1, 2, 16} and test_inflight_algorithm.py's
durations.  The same program also runs once under AddressSanitizer and
UBSan: it is host code with its own main.  CPU only: the GPU tests check the
kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "admit_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "admit_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


def _build(out, extra):
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_admit.h", "cg_profile.h", "cg_expand.h", "cg_time.h",
                                                    "cg_zone.h")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-o", out] + extra + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def admit_host():
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
    tail = out.stdout.split(" events checked, ")[1]
    walked = int(tail.split()[0])
    unit_walks, plain, dropped = (int(tail.split("; ")[1].split()[0]), int(tail.split(" unit walks, ")[1].split()[0]),
                                  int(tail.split(" drop, ")[1].split()[0]))
    # the walk ran and skipped, the shortcut was taken, fires were dropped
    assert unit_walks > 0 and plain > 0 and dropped > 0, out.stdout[-500:]
    if zone in WALKED:
        assert walked > 0, out.stdout[-500:]


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_admission_matches_the_literal_process(admit_host, zone):
    out = subprocess.run([admit_host, zone, "60", "11", "150000"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    _check(out, zone)


def test_host_admission_under_sanitizers():
    """The stand-alone program built with -fsanitize=address,undefined, on the
    zone with the most walked runs and a smaller fire budget."""
    binary = _build(BIN + "_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([binary, "Pacific/Chatham", "40", "11", "60000"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    _check(out, "Pacific/Chatham")
