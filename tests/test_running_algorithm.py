"""The routines a running profile call runs (cg_profile.h: the in-flight base
rows and running_emit_diff; cg_admit.h: admit_walk_unit; cg_lock.h:
lock_walk_unit -- the walks with the difference emit, then a host row scan in
k_rows_prefix's place), compiled for the host and checked cell by cell, in both
flavours, against the literal process of the definition run over the oracle's
Next loop and lockTtl (tests/native/running_host.cpp).  Zones, specs, t0
choices, shapes and unit sizes are test_admit_algorithm.py's; the admission
flavour runs its P values and durations, the lock flavour
test_lock_algorithm.py's kinds, AvgTimes, lock_ttl cycle and non-contending
rules.  Every cell is also held to running <= in flight.  The same program
runs once under AddressSanitizer and UBSan: it is host code with its own main.
CPU only: the GPU tests check the kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "running_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "running_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


def _build(out, extra):
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_lock.h", "cg_admit.h", "cg_profile.h", "cg_expand.h", "cg_time.h",
                                                    "cg_zone.h")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-o", out] + extra + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return out


@pytest.fixture(scope="module")
def running_host():
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

    def num(before):
        return int(last.split(before)[0].split()[-1])
    # both walks ran and skipped, the shortcut was taken, differences were
    # written, and the result is not just the in-flight profile again
    for what in (" admission walks", " units that never drop", " fires dropped", " lock walks", " fires granted",
                 " fires skipped", " differences written", " cells below in flight"):
        assert num(what) > 0, (what, last)
    if zone in WALKED:
        assert num(" of them walked") > 0, last


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_running_matches_the_literal_process(running_host, zone):
    out = subprocess.run([running_host, zone, "60", "11", "150000"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    _check(out, zone)


def test_host_running_under_sanitizers():
    """The stand-alone program built with -fsanitize=address,undefined, on the
    zone with the most walked runs and a smaller fire budget."""
    binary = _build(BIN + "_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([binary, "Pacific/Chatham", "40", "11", "60000"], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    _check(out, "Pacific/Chatham")
