#!/usr/bin/env python3
"""Measure the fire profile (cg_profile_device / cg_profile_per_node_device)
against the only route to the same numbers without it: one window per bucket.

  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the rule matrix.
           Parent route: B cg_expand_device_async windows of one bucket width,
           each waited for, its rule counts read off the window's offsets.
  config3  1M jobs x 10k nodes x 24 h, B = 24 one-hour buckets: the node
           matrix.  Parent route: B pipelined per-node windows
           (cg_expand_per_node_rules_device_async) of one bucket width, each
           waited for, its per-node counts read off the window's node offsets
           (cg_node_counts_to_device).

(A window's offsets are readable only after its wait, so the parent route
cannot keep windows in flight.)  A window anchors an `@every` rule at its own
start, the profile at t0, so the parent route does not give the same numbers
for `@every` rules whose delay does not divide the bucket width: config2
compares the rows of the other rules (and records how many `@every` rows
differ), config3 snaps every `@every` delay to a divisor of the one-hour
bucket (at most one hour), so that every node's row must agree.  Both routes run in this process, alternating,
--pairs times each; the two results are asserted equal before anything is
timed.  Route times are wall ms around calls that end in a stream
synchronise; the profile's kernels are timed by HIP events on the engine's
stream (cg_last_kernel_times).  Bytes are algorithmic: computed from the
shapes, not measured.  One JSON line per shape goes to --out.

Run by hand on an MI355X:
    python tools/profile_bench.py --out profiles/profile_bench.json
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

SPEC_BYTES, RUN_BYTES = 32, 20  # a packed spec; a run record {anchor, count, daymask}


class _View:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


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


DIVISORS_3600 = [d for d in range(30, 3601) if 3600 % d == 0]


def every_seconds(spec):
    d, n = 0, ""
    for ch in spec[len("@every "):]:
        if ch.isdigit():
            n += ch
        else:
            d += int(n) * {"h": 3600, "m": 60, "s": 1}[ch]
            n = ""
    return d


def upload(eng, R, seed, mix, snap_every=False):
    specs = synth.spec_mix(R, seed=seed, mix=mix)
    if snap_every:  # the largest divisor of 3600 s that is at most the delay
        specs = [f"@every {max(x for x in DIVISORS_3600 if x <= max(every_seconds(s), 30))}s"
                 if s.startswith("@every") else s for s in specs]
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    return eng.upload_c(arr, R), specs


def verdict(new, old):
    spread = old["max"] - old["min"]
    return {"parent_minus_profile_median_ms": old["median"] - new["median"], "parent_spread_ms": spread,
            "faster_by_more_than_parent_spread": old["min"] - new["max"] > spread}


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    utc = cron.UTC()
    sp, specs = upload(eng, R, 0x5EED, synth.MIX_CONFIG2)
    dev = torch.device("cuda", 0)
    every = torch.tensor([s.startswith("@every") for s in specs], device=dev)
    cols = torch.zeros((B, R), dtype=torch.int32, device=dev)  # the parent route's [B][R]
    sync = torch.cuda.synchronize
    eng.expand_device(sp, utc, t0, t0 + 4 * w)  # sizes the windows' output
    eng.set_phase_timing(1)

    def old():
        for b in range(B):
            eng.expand_async(sp, utc, t0 + b * w, t0 + (b + 1) * w)
            eng.expand_wait()
            off = torch.as_tensor(_View(eng.result_device()[0], R + 1, "<i8"), device=dev)
            torch.sub(off[1:], off[:-1], out=cols[b])
            if b & 1:  # a window set's offsets are rewritten three calls on
                sync()
        sync()

    out = {}

    def new():
        out["rules"], out["totals"] = eng.profile_device(sp, utc, t0, w, B)

    old()
    new()
    sync()
    differ = (out["rules"] != cols.t()).any(dim=1)
    assert not bool((differ & ~every).any()), "profile and per-window counts differ"
    assert torch.equal(out["totals"], out["rules"].sum(dim=0, dtype=torch.int64))
    n_every, n_every_differ = int(every.sum()), int(differ.sum())
    del differ
    E = int(out["totals"].sum())
    eng.set_phase_timing(2)
    new()
    kt, ct = eng.profile_kernel_times(), eng.kernel_times()
    eng.set_phase_timing(1)
    a, b = alternate(new, old, args.pairs, sync)
    new_s, old_s = stats(a), stats(b)
    G = 1  # UTC, 24 h: one closed-form segment
    return {"shape": "config2 rule matrix", "rules": R, "width_s": w, "buckets": B, "fires": E,
            "routes_equal": f"on the {R - n_every} rules that are not @every; {n_every_differ} of the {n_every} "
            "@every rows differ (a window re-anchors @every at its start)",
            "pairs": args.pairs, "order": "alternating, profile first in even pairs",
            "profile_ms": new_s, "parent_ms": old_s, "parent_route": f"{B} cg_expand_device_async windows, each waited "
            "for, counts = offsets[1:] - offsets[:-1] on the device",
            "profile_kernels_ms": {"k_count": ct[0], "scan": ct[1], "k_profile_rules": kt[0], "k_profile_walk": kt[1],
                                   "k_profile_totals": kt[2]},
            "algorithmic_bytes": {"k_profile_rules": R * SPEC_BYTES + R * G * RUN_BYTES + R * B * 4,
                                  "k_profile_totals": R * B * 4 + B * 8,
                                  "parent_route_stores": E * 8 + B * (R + 1) * 8},
            **verdict(new_s, old_s)}


def config3(eng, torch, args):
    R, w, B, t0, N = args.rules, 3600, 24, synth.T0_2026, 10_000
    utc = cron.UTC()
    sp, _ = upload(eng, R, 0x5EED + 3, synth.MIX_CONFIG2, snap_every=True)
    rin = synth.rules_for_nodes(R, n_nodes=N, n_groups=500, seed=0x5EED + 3)
    dr = eng.upload_rules(rin)
    mode = _lib.EXCLUDE_NONE
    dev = torch.device("cuda", 0)
    cols = torch.zeros((B, N), dtype=torch.int64, device=dev)
    sync = torch.cuda.synchronize
    nnz = 0
    for b in range(B):  # synchronous windows size the outputs for the pipelined ones
        _, nnz = eng.expand_per_node_rules_device(sp, utc, t0 + b * w, t0 + (b + 1) * w, dr, mode)

    def old():
        for b in range(B):
            eng.expand_per_node_async(sp, utc, t0 + b * w, t0 + (b + 1) * w, dr, mode)
            eng.expand_per_node_wait()
            eng.node_counts_to_device(cols[b].data_ptr())

    out = {}

    def new():
        out["rules"], out["totals"], out["nodes"] = eng.profile_per_node_device(sp, utc, t0, w, B, dr, mode)

    old()
    new()
    sync()
    assert torch.equal(out["nodes"], cols.t()), "node profile and per-window node counts differ"
    En = int(out["nodes"].sum())
    eng.set_phase_timing(2)
    new()
    kt, ct = eng.profile_kernel_times(), eng.kernel_times()
    a, b = alternate(new, old, args.pairs, sync)
    new_s, old_s = stats(a), stats(b)
    return {"shape": "config3 node matrix (@every delays snapped to divisors of 3600 s)", "rules": R, "nodes": N, "join_pairs": nnz, "width_s": w, "buckets": B,
            "node_fires": En, "routes_equal": True, "pairs": args.pairs,
            "order": "alternating, profile first in even pairs", "profile_ms": new_s, "parent_ms": old_s,
            "parent_route": f"{B} cg_expand_per_node_rules_device_async windows, each waited for, counts by "
            "cg_node_counts_to_device",
            "profile_kernels_ms": {"k_count": ct[0], "scan": ct[1], "k_profile_rules": kt[0], "k_profile_walk": kt[1],
                                   "k_profile_totals": kt[2], "join_and_transpose": kt[3],
                                   "k_profile_nodes": kt[4]},
            "algorithmic_bytes": {"k_profile_rules": R * SPEC_BYTES + R * RUN_BYTES + R * B * 4,
                                  "k_profile_totals": R * B * 4 + B * 8,
                                  "k_profile_nodes": nnz * 4 + nnz * B * 4 + N * B * 8,
                                  "parent_route_stores": En * 12},
            **verdict(new_s, old_s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
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
