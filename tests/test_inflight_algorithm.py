"""The in-flight profile algorithm the kernels run (cg_profile.h: inflight_cell
at every bucket edge over the run records of count_rule, and the two-cursor
sweep inflight_walk_row for walked runs), compiled for the host and checked
cell by cell against the oracle's literal Next loop, its fires counted directly
from the duration in milliseconds (tests/native/inflight_host.cpp).  Zones,
specs, t0 choices and shapes are test_profile_algorithm.py's; every rule is
checked with durations of 0, 1, 999, 1000, 1001 ms, w*1000 - 1, w*1000,
w*1000 + 1, 3.5 w, 45 days and INT64_MAX ms.  CPU only: the GPU tests check
the kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "inflight_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "inflight_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


@pytest.fixture(scope="module")
def inflight_host():
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_profile.h", "cg_expand.h", "cg_time.h", "cg_zone.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(BIN) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", BIN] + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return BIN


# zones whose 2026 transitions leave walked runs inside the checked horizons
WALKED = {"America/Havana", "Australia/Lord_Howe", "Pacific/Chatham"}


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_inflight_matches_counted_oracle(inflight_host, zone):
    out = subprocess.run([inflight_host, zone, "60", "11"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout
    # horizons the oracle reports as non-terminating are skipped and counted:
    # at most a quarter of a zone's may be
    line = [l for l in out.stdout.splitlines() if "horizons skipped" in l][0]
    print(line)
    skipped, n_all = int(line.split(": ")[1].split()[0]), int(line.split(" of ")[1].split()[0])
    assert n_all >= 8 and 4 * skipped <= n_all, line
    # the sweep ran: walked fires were among the checked ones
    walked = int(out.stdout.split(" events checked, ")[1].split()[0])
    if zone in WALKED:
        assert walked > 0, out.stdout[-500:]
