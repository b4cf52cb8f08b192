"""bench.py's plain run, `--full` and `--dump-outputs DIR`.

A plain run sets up, warms up, times `--steps` steps and prints the line;
the oracle check, the CPU baseline and the other measurements around the
timed region come with `--full`.  `--dump-outputs DIR` writes what the last
timed step left for its caller as DIR/<name>.npy in float64.  The GPU test
runs a small config-2 shaped workload (5000 rules x 1 h, below the dump's
sampling threshold, so the whole result is written) and compares the files
with the oracle's expansion of the same seeded rules."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, BENCH] + list(args), capture_output=True, text=True, timeout=timeout,
                          env=env, cwd=ROOT)


def test_dump_outputs_refused_for_the_host_only_workload(tmp_path):
    p = _bench("--workload", "parse", "--dump-outputs", str(tmp_path / "d"))
    assert p.returncode == 2
    assert "--dump-outputs" in p.stderr and p.stdout.strip() == ""
    assert not (tmp_path / "d").exists()


def test_full_is_an_option_and_off_by_default():
    p = _bench("--help")
    assert p.returncode == 0
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = _bench("--gpus", "2", "--dry-run", "--full")  # accepted beside the launcher's options
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip()) == {"dry_run": True, "rank": 0, "world": 2, "gpus": 2}


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_result(tmp_path):
    import oracle_lib as O
    from cronsun_amd import synth
    R, H, steps = 5000, 3600, 3
    out = tmp_path / "dump"
    p = _bench("--gpus", "1", "--steps", str(steps), "--warmup", "1", "--rules", str(R), "--horizon", str(H),
               "--dump-outputs", str(out))
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d
    assert d["steps"] == steps and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    # a plain run: nothing checked or measured beside the timed steps
    assert d["full"] is False and d["verified"] is None and d["verify"] is None
    assert d["cpu_baseline"] is None and d["roofline"]["store_ceiling"] is None and "end_to_end_rank0" not in d
    E = d["config"]["events_per_gpu_step"]
    assert d["value"] * d["ms_per_step"] / 1e3 == pytest.approx(E, rel=1e-9)  # events/s over the timed steps

    specs = synth.spec_mix(R, seed=0x5EED, mix=synth.MIX_CONFIG2)  # the benchmark's config-2 rules
    arr = O.sched_array([O.parse(s)[0] for s in specs])
    eo, et = O.expand_batch(arr, synth.T0_2026, synth.T0_2026 + H, O.Loc("UTC"))
    assert sorted(os.listdir(out)) == ["offsets.npy", "times.npy"]
    off, times = np.load(out / "offsets.npy"), np.load(out / "times.npy")
    assert off.dtype == np.float64 and times.dtype == np.float64
    assert E == int(eo[-1]) and d["dumped_outputs"] == {"events": E, "sampled": False,
                                                       "files": {"offsets.npy": R + 1, "times.npy": E}}
    assert np.array_equal(off, eo.astype(np.float64))
    assert np.array_equal(times, et.astype(np.float64))
