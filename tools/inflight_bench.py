#!/usr/bin/env python3
"""Measure the in-flight profile (cg_inflight_device /
cg_inflight_per_node_device) against the start profile of the same shape on
the same box -- the baseline it shares its chain with; no ratio is set in
advance.

  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the rule matrix.
  config3  1M jobs x 10k nodes x 24 h, B = 24 one-hour buckets: the node
           matrix (and, once, its row peaks).

Durations are drawn from a seed, log-uniform from 1 ms to 2 h.  Before
anything is timed the results are held to the identities of the definition on
the device: a duration of one width gives the start profile, 0 ms nothing,
INT64_MAX ms the prefix sums of the start rows, the totals are the column
sums, and with the seeded durations every row is bounded by its prefix sums.
Both calls run in this process, alternating, --pairs times each after two
warm-ups; times are wall ms around calls that end in a stream synchronise, the
kernels are timed by HIP events on the engine's stream
(cg_last_kernel_times [14..18]).  One JSON line per shape goes to --out.

Run by hand on an MI355X:
    python tools/inflight_bench.py --out profiles/inflight_bench.json
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

from cronsun_amd import _lib, cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402

INT64_MAX = (1 << 63) - 1
KERNELS = ("k_inflight_rules", "k_inflight_walk", "k_profile_totals", "join_and_transpose", "k_profile_nodes")
START_KERNELS = ("k_profile_rules", "k_profile_walk", "k_profile_totals", "join_and_transpose", "k_profile_nodes")


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


def durations(R, seed):
    """int64 [R] ms, log-uniform over [1 ms, 2 h]."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(0.0, np.log(7_200_000.0), R)).astype(np.int64).clip(1, 7_200_000)


def upload(eng, R, seed):
    arr, status = cron.parse_batch(synth.spec_mix(R, seed=seed, mix=synth.MIX_CONFIG2), threads=16)
    assert (status == 0).all()
    return eng.upload_c(arr, R)


def check_identities(torch, call, starts, w, R):
    """call(dur_ms) -> (rules, totals) views; starts: a copy of the start matrix."""
    rules, totals = call(np.full(R, w * 1000, dtype=np.int64))
    assert torch.equal(rules, starts), "a duration of one width is not the start profile"
    assert torch.equal(totals, starts.sum(dim=0, dtype=torch.int64))
    rules, totals = call(np.zeros(R, dtype=np.int64))
    assert not bool(rules.any()) and not bool(totals.any()), "0 ms is in flight"
    pre = torch.cumsum(starts, dim=1, dtype=torch.int32)
    rules, totals = call(np.full(R, INT64_MAX, dtype=np.int64))
    assert torch.equal(rules, pre), "INT64_MAX ms is not the prefix sums"
    return pre


def measure(eng, torch, args, new, old, n_kernels):
    sync = torch.cuda.synchronize
    for _ in range(2):  # warm-ups
        new()
        old()
    sync()
    new()
    kt_new = eng.profile_kernel_times()[:n_kernels]
    old()
    kt_old = eng.profile_kernel_times()[:n_kernels]
    a, b = alternate(new, old, args.pairs, sync)
    return stats(a), stats(b), kt_new, kt_old


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    utc = cron.UTC()
    sp = upload(eng, R, 0x5EED)
    dur = durations(R, args.seed)
    starts = eng.profile_device(sp, utc, t0, w, B)[0].clone()
    pre = check_identities(torch, lambda d: eng.inflight_device(sp, utc, t0, w, B, d), starts, w, R)
    rules, totals = eng.inflight_device(sp, utc, t0, w, B, dur)
    assert bool((rules <= pre).all()) and torch.equal(totals, rules.sum(dim=0, dtype=torch.int64))
    in_flight_max = int(totals.max())
    del starts, pre, rules, totals
    torch.cuda.empty_cache()
    new_s, old_s, kt_new, kt_old = measure(eng, torch, args, lambda: eng.inflight_device(sp, utc, t0, w, B, dur),
                                           lambda: eng.profile_device(sp, utc, t0, w, B), 3)
    return {"shape": "config2 rule matrix", "rules": R, "width_s": w, "buckets": B, "duration_seed": args.seed,
            "durations_ms": "log-uniform 1 .. 7 200 000", "largest_cluster_in_flight": in_flight_max,
            "identities": "d = w, 0 ms, INT64_MAX ms, totals = column sums, rows <= prefix sums: exact",
            "pairs": args.pairs, "warmups": 2, "order": "alternating, in-flight first in even pairs",
            "inflight_ms": new_s, "start_profile_ms": old_s,
            "inflight_kernels_ms": dict(zip(KERNELS, kt_new)), "start_profile_kernels_ms": dict(zip(START_KERNELS, kt_old)),
            "inflight_minus_start_median_ms": new_s["median"] - old_s["median"],
            "start_profile_spread_ms": old_s["max"] - old_s["min"]}


def config3(eng, torch, args):
    R, w, B, t0, N = args.rules, 3600, 24, synth.T0_2026, 10_000
    utc = cron.UTC()
    sp = upload(eng, R, 0x5EED + 3)
    dr = eng.upload_rules(synth.rules_for_nodes(R, n_nodes=N, n_groups=500, seed=0x5EED + 3))
    mode = _lib.EXCLUDE_NONE
    dur = durations(R, args.seed + 3)
    starts, _, start_nodes = [x.clone() for x in eng.profile_per_node_device(sp, utc, t0, w, B, dr, mode)]

    def call(d):
        rules, totals, nodes = eng.inflight_per_node_device(sp, utc, t0, w, B, d, dr, mode)
        call.nodes = nodes
        return rules, totals
    check_identities(torch, call, starts, w, R)
    assert torch.equal(call.nodes, torch.cumsum(start_nodes, dim=1)), "node matrix of INT64_MAX ms"
    rules, totals, nodes = eng.inflight_per_node_device(sp, utc, t0, w, B, dur, dr, mode)
    assert torch.equal(totals, rules.sum(dim=0, dtype=torch.int64))
    sync = torch.cuda.synchronize
    peaks_ms = timed(eng.profile_node_peaks, sync)  # first use: the kernel, its synchronise and two copies
    peak, bucket = eng.profile_node_peaks()
    host = nodes.cpu().numpy()
    assert np.array_equal(peak, host.max(axis=1)) and np.array_equal(bucket, host.argmax(axis=1))
    del starts, start_nodes, rules, totals, nodes
    new_s, old_s, kt_new, kt_old = measure(
        eng, torch, args, lambda: eng.inflight_per_node_device(sp, utc, t0, w, B, dur, dr, mode),
        lambda: eng.profile_per_node_device(sp, utc, t0, w, B, dr, mode), 5)
    return {"shape": "config3 node matrix", "rules": R, "nodes": N, "width_s": w, "buckets": B,
            "duration_seed": args.seed + 3, "durations_ms": "log-uniform 1 .. 7 200 000",
            "largest_node_peak": int(peak.max()),
            "identities": "d = w, 0 ms, INT64_MAX ms (rule and node matrix), totals = column sums, peaks = "
            "max / first argmax: exact",
            "pairs": args.pairs, "warmups": 2, "order": "alternating, in-flight first in even pairs",
            "inflight_ms": new_s, "start_profile_ms": old_s, "node_peaks_first_use_wall_ms": peaks_ms,
            "inflight_kernels_ms": dict(zip(KERNELS, kt_new)), "start_profile_kernels_ms": dict(zip(START_KERNELS, kt_old)),
            "inflight_minus_start_median_ms": new_s["median"] - old_s["median"],
            "start_profile_spread_ms": old_s["max"] - old_s["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflight_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0xD0)
    ap.add_argument("--shapes", default="config2,config3")
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("at least five pairs")
    import torch
    eng = Engine(0)
    lines = []
    for name in args.shapes.split(","):
        rec = {"config2": config2, "config3": config3}[name](eng, torch, args)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # kept after every shape
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    eng.close()


if __name__ == "__main__":
    main()
