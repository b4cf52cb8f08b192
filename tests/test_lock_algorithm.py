"""The lock routine the kernel runs (cg_lock.h: lock_walk_unit over the run
records of count_rule, with admit_fire_after's closed forms, walked runs and
skips, and two next_exact calls past the horizon per fire that finds the key
gone, over the zone table a lock profile stages), compiled for the host and
checked cell by cell, in both kinds, against the literal process of the
definition run over the oracle's Next loop with the oracle's or_lock_ttl
(tests/native/lock_host.cpp).  Zones, specs, t0 choices and shapes are
test_admit_algorithm.py's; the rules of a horizon form units of 1, 2, 5 and 9,
each checked as ALONE and INTERVAL with avg_ms in {0, 999, 1000, 2500, 60000,
3600000, -1500, INT64_MAX}; lock_ttl in {2, 300, 600} and a non-contending
first, middle or last rule cycle over the combinations.  A fire whose Next
never returns (Pacific/Apia's skipped day) must be reported as the oracle
reports it.  The same program also runs once under AddressSanitizer and UBSan:
it is host code with its own main.  CPU only: the GPU tests check the kernel
itself."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lock_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "lock_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


def _build(out, extra):
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_lock.h", "cg_admit.h", "cg_profile.h", "cg_expand.h",
                                                    "cg_time.h", "cg_zone.h")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-o", out] + extra + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def lock_host():
    return _build(BIN, ["-O2"])


# zones whose 2026 transitions leave walked runs inside the checked horizons
WALKED = {"America/Havana", "Australia/Lord_Howe", "Pacific/Chatham"}


def _num(text, after):
    return int(re.search(r"(\d+) " + re.escape(after), text).group(1))


def _check(out, zone):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout
    # horizons the oracle reports as non-terminating are skipped and counted:
    # at most a quarter of a zone's may be
    line = [l for l in out.stdout.splitlines() if "horizons skipped" in l][0]
    print(line)
    print(out.stdout.splitlines()[-1])
    skipped, n_all = int(line.split(": ")[1].split()[0]), int(line.split(" of ")[1].split()[0])
    assert n_all >= 8 and 4 * skipped <= n_all, line
    s = out.stdout
    # fires were granted and skipped, the walk jumped ahead, and ttls came from Next calls past t1
    for what in ("unit walks", "fires granted", "fires skipped", "skip-ahead jumps", "with a Next past t1"):
        assert _num(s, what) > 0, (what, s[-600:])
    if zone in WALKED:
        assert _num(s, "of them walked") > 0, s[-600:]


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_lock_walk_matches_the_literal_process(lock_host, zone):
    # (a smaller fire budget than the admission check's: every fire is visited in 64 combinations, each
    # asking the oracle's lockTtl -- two literal Next loops -- where it finds the key gone)
    out = subprocess.run([lock_host, zone, "60", "11", "10000"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    _check(out, zone)


def test_a_next_that_never_returns_is_reported(lock_host):
    """Pacific/Apia, the days before the skipped 2011-12-30: the expansion
    ends, but the second Next from a granted fire does not."""
    out = subprocess.run([lock_host, "Pacific/Apia"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout and _num(out.stdout, "walks the oracle's lockTtl never returns from") > 0


def test_host_lock_walk_under_sanitizers():
    """The stand-alone program built with -fsanitize=address,undefined, on the
    zone with the most walked runs and a smaller fire budget, and the stuck case."""
    binary = _build(BIN + "_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([binary, "Pacific/Chatham", "40", "11", "3000"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    _check(out, "Pacific/Chatham")
    out = subprocess.run([binary, "Pacific/Apia"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
