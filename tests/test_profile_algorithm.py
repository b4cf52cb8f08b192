"""The fire-profile algorithm the kernels run (cg_profile.h: per bucket, the
difference of run_fires_upto at the clipped bucket edges over the run records
of count_rule, plus next_exact for walked runs), compiled for the host and
checked cell by cell against the oracle's literal Next loop binned by
(t - t0 - 1) // width (tests/native/profile_host.cpp): random specs, every
second, @every delays that divide no bucket width, a rule that never fires;
t0 at a non-aligned second, plain and around the first two transitions of
2026; (width, buckets) from 130 one-second buckets to 14 weeks (98 days, so
buckets straddle the 30-day segment cuts).  CPU only: the GPU tests check the
kernels themselves."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "profile_host.cpp")
BIN = os.path.join(ROOT, "tests", "native", "profile_host")
CSRC = os.path.join(ROOT, "cronsun_amd", "csrc")


@pytest.fixture(scope="module")
def profile_host():
    import oracle_lib as O
    O.lib()  # builds oracle/liboracle.so if needed
    srcs = [SRC, os.path.join(CSRC, "cg_zone.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("cg_profile.h", "cg_expand.h", "cg_time.h", "cg_zone.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(BIN) < os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", BIN] + srcs +
                              ["-L" + os.path.join(ROOT, "oracle"), "-loracle",
                               "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return BIN


@pytest.mark.parametrize("zone", ["UTC", "America/New_York", "Europe/London", "America/Havana",
                                  "Australia/Lord_Howe", "Pacific/Chatham", "Africa/Casablanca"])
def test_host_profile_matches_binned_oracle(profile_host, zone):
    out = subprocess.run([profile_host, zone, "60", "11"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout
    # horizons the oracle reports as non-terminating are skipped and counted:
    # at most a quarter of a zone's may be
    line = [l for l in out.stdout.splitlines() if "horizons skipped" in l][0]
    skipped, n_all = int(line.split(": ")[1].split()[0]), int(line.split(" of ")[1].split()[0])
    assert n_all >= 8 and 4 * skipped <= n_all, line
