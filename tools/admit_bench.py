#!/usr/bin/env python3
"""Measure the admission profile (cg_admit_device, kind ADMITTED) against the
start profile of the same shape on the same box -- the chain it extends by
two kernels; no ratio is set in advance.

  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the rule matrix.

Every rule is its own unit.  Durations are drawn from a seed, log-uniform from
1 ms to 2 h; Parallels from the same seed, 0, 1 or 2 with the shares recorded.
Before anything is timed the results are held to the definition on the device:
admitted + dropped is the start profile cell by cell, Parallels 0 everywhere
and 0 ms everywhere admit every fire, the totals are the column sums, and no
rule is admitted more than its start row.  Both calls run in this process,
alternating, --pairs times each after two warm-ups; times are wall ms around
calls that end in a stream synchronise, the kernels are timed by HIP events on
the engine's stream (cg_last_kernel_times [14..16], [19..20]).  The record
names the share of units that could drop and the longest lane of k_admit_units
(the unit with the most admitted fires: a lane steps once per admitted fire).

Run by hand on an MI355X:
    python tools/admit_bench.py --out profiles/admit_bench.json
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

from cronsun_amd import cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402

START_KERNELS = ("k_profile_rules", "k_profile_walk", "k_profile_totals")
ADMIT_KERNELS = START_KERNELS + ("k_admit_prepare", "k_admit_units")


def stats(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "all": [round(x, 4) for x in ms]}


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def alternate(new, old, pairs, sync):
    a, b = [], []
    for i in range(pairs):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (a if which == 0 else b).append(timed(new if which == 0 else old, sync))
    return a, b


def draw(R, seed, shares):
    """(dur_ms int64 [R] log-uniform over [1 ms, 2 h], parallels int64 [R] in {0, 1, 2})."""
    rng = np.random.default_rng(seed)
    dur = np.exp(rng.uniform(0.0, np.log(7_200_000.0), R)).astype(np.int64).clip(1, 7_200_000)
    par = rng.choice(np.array([0, 1, 2], dtype=np.int64), R, p=shares)
    return dur, par


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    utc = cron.UTC()
    specs = synth.spec_mix(R, seed=0x5EED, mix=synth.MIX_CONFIG2)
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    sp = eng.upload_c(arr, R)
    shares = [float(x) for x in args.parallels_shares.split(",")]
    dur, par = draw(R, args.seed, shares)
    zeros = np.zeros(R, dtype=np.int64)
    call = lambda d, p, what: eng.admit_device(sp, utc, t0, w, B, d, p, None, what=what)  # noqa: E731

    starts = eng.profile_device(sp, utc, t0, w, B)[0].clone()
    rules, totals = call(dur, zeros, "admitted")
    assert torch.equal(rules, starts), "Parallels 0 does not admit every fire"
    rules, totals = call(zeros, par, "dropped")
    assert not bool(rules.any()) and not bool(totals.any()), "0 ms drops"
    dropped = call(dur, par, "dropped")[0].clone()
    rules, totals = call(dur, par, "admitted")
    assert torch.equal(rules + dropped, starts), "admitted + dropped is not the start profile"
    assert bool((rules >= 0).all()) and bool((dropped >= 0).all())
    assert torch.equal(totals, rules.sum(dim=0, dtype=torch.int64))
    # units that could drop, and the longest lane: one step per admitted fire
    d_sec = np.minimum(dur // 1000 + (dur % 1000 != 0), w * B)
    could = (par > 0) & (d_sec > par)
    admitted_per_rule = rules.sum(dim=1, dtype=torch.int64).cpu().numpy()
    lane = int(np.argmax(np.where(could, admitted_per_rule, -1)))
    n_dropped, n_starts = int(dropped.sum()), int(starts.sum())
    every_second = np.array([s == "* * * * * *" for s in specs])
    del starts, dropped, rules, totals
    torch.cuda.empty_cache()

    sync = torch.cuda.synchronize
    new = lambda: call(dur, par, "admitted")  # noqa: E731
    old = lambda: eng.profile_device(sp, utc, t0, w, B)  # noqa: E731
    for _ in range(2):  # warm-ups
        new()
        old()
    sync()
    new()
    kt_new = eng.profile_kernel_times()[:3] + eng.admit_kernel_times()
    old()
    kt_old = eng.profile_kernel_times()[:3]
    a, b = alternate(new, old, args.pairs, sync)
    new_s, old_s = stats(a), stats(b)
    return {"shape": "config2 rule matrix", "rules": R, "width_s": w, "buckets": B, "seed": args.seed,
            "units": "every rule its own unit", "durations_ms": "log-uniform 1 .. 7 200 000",
            "parallels_shares_0_1_2": shares,
            "units_that_could_drop": int(could.sum()), "share_of_units_that_could_drop": float(could.mean()),
            "every_second_rules": int(every_second.sum()),
            "every_second_rules_that_could_drop": int((every_second & could).sum()),
            "fires": n_starts, "fires_dropped": n_dropped,
            "longest_lane": {"rule": lane, "spec": specs[lane], "admitted_fires": int(admitted_per_rule[lane]),
                             "dur_ms": int(dur[lane]), "parallels": int(par[lane])},
            "identities": "admitted + dropped = starts, Parallels 0 and 0 ms admit all, totals = column sums: exact",
            "pairs": args.pairs, "warmups": 2, "order": "alternating, admitted first in even pairs",
            "admitted_ms": new_s, "start_profile_ms": old_s,
            "admitted_kernels_ms": dict(zip(ADMIT_KERNELS, kt_new)),
            "start_profile_kernels_ms": dict(zip(START_KERNELS, kt_old)),
            "admitted_minus_start_median_ms": new_s["median"] - old_s["median"],
            "start_profile_spread_ms": old_s["max"] - old_s["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0xAD)
    ap.add_argument("--parallels-shares", default="0.5,0.3,0.2", help="shares of Parallels 0, 1 and 2")
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
