#!/usr/bin/env python3
"""Measure the fire verdicts (cg_expand_verdicts_device) against the two calls
that do the same expansion and the same walk on the same box; no target is set
in advance.

  config2  1M mixed rules x 24 h, UTC.  Admission mix: tools/admit_bench.py's
           (durations log-uniform 1 ms .. 2 h, Parallels 0 / 1 / 2); lock mix:
           tools/lock_bench.py's (kinds COMMON / ALONE / INTERVAL, AvgTime
           log-uniform 1 ms .. 2 h, LockTtl 300).  Every rule is its own unit.

  admission-only verdict call   vs   expand_device, then admit(what="dropped",
                                     width=60, n_buckets=1440)
  lock-only verdict call        vs   expand_device, then lock_runs(what="skipped")

Before anything is timed the bytes are held to the profiles on the device: the
fires with bit 0, binned into the 1440 buckets, are the DROPPED matrix cell by
cell and those without it the ADMITTED one; the same for bit 1 against SKIPPED /
GRANTED.  Both sides run in this process, alternating, --pairs times each after
two warm-ups; times are wall ms around calls that end in a stream synchronise.
The phases are timed by HIP events on the engine's stream (cg_verdict_times):
expansion, init pass, admission walk, lock walk, and for the selection (1, 1)
its count + scan and its write.  After every timed call the event time of its
unit walk is read too (k_admit_verdicts / k_lock_verdicts, and the profile
call's k_admit_units / k_lock_units), so the record says how much of each
side's wall time is the walk and how much is everything else.

Run by hand on an MI355X:
    python tools/verdict_bench.py --out profiles/verdict_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import admit_bench  # noqa: E402
import lock_bench  # noqa: E402
from cronsun_amd import _lib, cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402

PHASES = ("expansion", "k_verdict_init", "k_admit_verdicts", "k_lock_verdicts", "select_count_scan", "select_write")


def stats(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "all": [round(x, 4) for x in ms]}


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def alternate(new, old, pairs, sync, walk_new, walk_old):
    """Wall ms of the two sides, alternating, and after every timed call the
    event time of its unit walk (read outside the timed interval)."""
    a, b, wa, wb = [], [], [], []
    for i in range(pairs):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (a if which == 0 else b).append(timed(new if which == 0 else old, sync))
            (wa if which == 0 else wb).append(walk_new() if which == 0 else walk_old())
    return a, b, wa, wb


def view(torch, dev, ptr, n, typestr):
    class _View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}
    return torch.as_tensor(_View(), device=dev)


def binned(torch, dev, eng, R, t0, w, B, bit, want_set):
    """int32 [R, B] on the device: the fires whose verdict has `bit` set
    (want_set) or clear, per rule and bucket, from the engine's own buffers."""
    d_off, d_times, n = eng.result_device()
    d_v, n1 = eng.verdicts_device()
    assert n1 == n
    off = view(torch, dev, d_off, R + 1, "<i8")
    times = view(torch, dev, d_times, n, "<i8")
    v = view(torch, dev, d_v, n, "|u1")
    keep = ((v & bit) != 0) if want_set else ((v & bit) == 0)
    rule = torch.repeat_interleave(torch.arange(R, device=dev), off[1:] - off[:-1])
    cell = rule[keep] * B + torch.div(times[keep] - t0 - 1, w, rounding_mode="floor")
    del rule, keep
    out = torch.bincount(cell, minlength=R * B).to(torch.int32).reshape(R, B)
    del cell
    return out


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    t1 = t0 + w * B
    utc = cron.UTC()
    dev = torch.device("cuda", eng.device)
    specs = synth.spec_mix(R, seed=0x5EED, mix=synth.MIX_CONFIG2)
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    sp = eng.upload_c(arr, R)
    dur, par = admit_bench.draw(R, args.admit_seed, [0.5, 0.3, 0.2])
    kind, avg = lock_bench.draw(R, args.lock_seed)
    admit, lock = (dur, par, None), (kind, avg, None, None, 300)

    # the identities, on the device
    E = eng.expand_verdicts_device(sp, utc, t0, t1, admit, None)
    got = {what: binned(torch, dev, eng, R, t0, w, B, _lib.VERDICT_DROPPED, what == "dropped")
           for what in ("dropped", "admitted")}
    for what in got:
        assert torch.equal(got[what], eng.admit_device(sp, utc, t0, w, B, dur, par, None, what=what)[0]), what
    n_dropped = int(got["dropped"].sum())
    del got
    eng.expand_verdicts_device(sp, utc, t0, t1, None, lock)
    got = {what: binned(torch, dev, eng, R, t0, w, B, _lib.VERDICT_SKIPPED, what == "skipped")
           for what in ("skipped", "granted")}
    for what in got:
        assert torch.equal(got[what], eng.lock_runs_device(sp, utc, t0, w, B, kind, avg, None, None, 300, what)[0]), what
    n_skipped = int(got["skipped"].sum())
    del got
    torch.cuda.empty_cache()

    sync = torch.cuda.synchronize
    rec = {"shape": "config2", "rules": R, "horizon_s": w * B, "fires": E, "fires_dropped": n_dropped,
           "fires_skipped": n_skipped, "units": "every rule its own unit",
           "admission_mix": "tools/admit_bench.py: durations log-uniform 1 .. 7 200 000 ms, Parallels 0/1/2 at "
                            "0.5/0.3/0.2",
           "lock_mix": "tools/lock_bench.py: kinds COMMON/ALONE/INTERVAL, AvgTime log-uniform 1 .. 7 200 000 ms, "
                       "LockTtl 300",
           "identities": "bit 0 set / clear binned = admit DROPPED / ADMITTED, bit 1 set / clear binned = lock_runs "
                         "SKIPPED / GRANTED, cell by cell on the device: exact",
           "pairs": args.pairs, "warmups": 2, "order": "alternating, the verdict call first in even pairs"}
    sides = {
        "admission": (lambda: eng.expand_verdicts_device(sp, utc, t0, t1, admit, None),
                      lambda: (eng.expand_device(sp, utc, t0, t1),
                               eng.admit_device(sp, utc, t0, w, B, dur, par, None, what="dropped"))),
        "lock": (lambda: eng.expand_verdicts_device(sp, utc, t0, t1, None, lock),
                 lambda: (eng.expand_device(sp, utc, t0, t1),
                          eng.lock_runs_device(sp, utc, t0, w, B, kind, avg, None, None, 300, "skipped"))),
    }
    for name, (new, old) in sides.items():
        for _ in range(2):  # warm-ups
            new()
            old()
        sync()
        new()
        n_sel = eng.verdicts_select_device(1 if name == "admission" else 2, 1 if name == "admission" else 2)
        phases = dict(zip(PHASES, eng.verdict_times()))
        old()
        own = eng.admit_kernel_times if name == "admission" else eng.lock_kernel_times
        parent = {"profile_kernels": eng.profile_kernel_times()[:3], "prepare_and_walk": own()}
        a, b, wa, wb = alternate(new, old, args.pairs, sync, lambda: eng.verdict_times()[2 if name == "admission" else 3],
                                 lambda: own()[1])
        new_s, old_s = stats(a), stats(b)
        rec[name] = {"verdict_call_ms": new_s, "parent_pair_ms": old_s, "verdict_phases_ms": phases,
                     "selected": n_sel, "parent_kernels_ms": parent,
                     "verdict_walk_kernel_ms": stats(wa), "parent_walk_kernel_ms": stats(wb),
                     "wall_minus_walk_ms": {"verdict": stats([x - y for x, y in zip(a, wa)]),
                                            "parent": stats([x - y for x, y in zip(b, wb)])},
                     "verdict_minus_parent_median_ms": new_s["median"] - old_s["median"],
                     "parent_pair_spread_ms": old_s["max"] - old_s["min"]}
    sp.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verdict_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--admit-seed", type=int, default=0xAD)
    ap.add_argument("--lock-seed", type=int, default=0x10C)
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("at least five pairs")
    import torch
    eng = Engine(0)
    rec = config2(eng, torch, args)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
