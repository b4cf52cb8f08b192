#!/usr/bin/env python3
"""Measure "what fires next" (cg_dispatcher_upcoming*) on the bench's dispatch
workload: synth.spec_mix entries (the 1M config-2 set, tiled past 1M as
bench.py does) bound to synth.rules_for_nodes over 10k nodes, started one
second before the top of an hour.

For k in 100, 4096, 65536, cluster-wide and for the node with the longest row
of the join, two routes in one process, alternating, after a warm-up of each
shape:
  device    cg_dispatcher_upcoming[_node] + cg_dispatcher_upcoming_copy: wall
            ms around the two calls (both end in a stream synchronise) and the
            device ms of the phases (cg_dispatcher_upcoming_times)
  snapshot  the only route before: cg_dispatcher_snapshot to the host, then
            the numpy selection of tests/upcoming_model.py
The two results are compared before anything is timed.  Each case reports
min / median / max of both routes over --reps repetitions, the streaming
passes the select took, and whether the slowest device call beats the fastest
snapshot call by more than the snapshot route's own spread.  Last, wakes of the
same table: cg_last_kernel_times[9] is k_dispatch_scan, one pass over the same
Next column -- the unit for "how many passes did the select cost".

Run by hand on an MI355X:
    python tools/dispatch_upcoming.py --out profiles/dispatch_upcoming.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cronsun_amd import _lib, cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402
from upcoming_model import upcoming  # noqa: E402

PHASES = ("select", "compaction", "sort_gather")


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def device_route(d, k, node):
    t = time.perf_counter()
    n, total = d.upcoming_count(k, None, node)
    cols = d.upcoming_copy(n)
    return (time.perf_counter() - t) * 1e3, cols, total


def snapshot_route(d, k, rows):
    t = time.perf_counter()
    nx, pv, _ = d.snapshot()
    t1 = time.perf_counter()
    s, a, b, total = upcoming(nx, pv, k, None, rows)
    t2 = time.perf_counter()
    return (t2 - t) * 1e3, (t1 - t) * 1e3, (s, a, b), total


def case(d, k, node, rows, reps, what):
    _, got, total = device_route(d, k, node)  # warm-up of this shape, and the comparison
    _, _, exp, etotal = snapshot_route(d, k, rows)
    same = total == etotal and all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert same, (what, k, "the device list differs from the snapshot route's")
    device_route(d, k, node)  # a second warm-up round, in the order that is timed
    snapshot_route(d, k, rows)
    dw, dd, ph, ps, sw, sc = [], [], [], [], [], []
    for _ in range(reps):
        w, _, _ = device_route(d, k, node)
        ms, passes = d.upcoming_ms()
        dw.append(w)
        dd.append(sum(ms))
        ph.append(ms)
        ps.append(passes)
        w, c, _, _ = snapshot_route(d, k, rows)
        sw.append(w)
        sc.append(c)
    best = min(range(reps), key=lambda i: dd[i])
    rec = {"scope": what, "k": k, "n_out": int(len(got[0])), "n_total": int(total),
           "candidates": int(len(d) if rows is None else len(rows)),
           "passes": sorted(set(ps)),
           "device": {"wall_ms": spread(dw), "device_ms": spread(dd),
                      "phase_ms_of_fastest": dict(zip(PHASES, ph[best]))},
           "snapshot": {"wall_ms": spread(sw), "copy_wall_ms": spread(sc)},
           "matches": bool(same)}
    rec["snapshot_spread_ms"] = max(sw) - min(sw)
    rec["fastest_snapshot_minus_slowest_device_ms"] = min(sw) - max(dw)
    rec["device_wins_by_more_than_snapshot_spread"] = bool(min(sw) - max(dw) > max(sw) - min(sw))
    print(json.dumps(rec), flush=True)
    return rec


def run_size(eng, R, n_nodes, reps, ks):
    utc = cron.UTC()
    base = synth.spec_mix(min(R, 1_000_000), seed=0x5EED + 5, mix=synth.MIX_CONFIG2)
    specs = (base * (R // len(base) + 1))[:R]
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    sp = eng.upload_c(arr, R)
    rin = synth.rules_for_nodes(R, n_nodes=n_nodes, n_groups=500, seed=0x5EED + 3)
    drules = eng.upload_rules(rin)
    hour = synth.T0_2026 + 10 * 3600
    d = eng.dispatcher(sp, utc, hour - 1)
    d.bind_rules(drules, _lib.EXCLUDE_NONE)
    # the node with the longest row, and the row (rules ascending)
    off, nodes = eng.rule_nodes(rin)
    node = int(np.argmax(np.bincount(nodes, minlength=n_nodes)))
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(off))[nodes == node]
    out = {"entries": R, "nodes": n_nodes, "nnz": int(len(nodes)), "longest_row_node": node,
           "longest_row": int(len(rows)), "cases": []}
    for k in ks:
        out["cases"].append(case(d, k, None, None, reps, "cluster"))
    for k in ks:
        out["cases"].append(case(d, k, node, rows, reps, "node"))
    # wakes of the same table: the scan is one pass over the same column
    scans = []
    for s in range(3):
        d.fire_count(hour + s)
        scans.append(eng.dispatch_kernel_times()[0])
    out["wake_scan_ms_kernel_times_9"] = scans
    for x in (d, drules, sp):
        x.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entries", type=int, nargs="+", default=[10_000_000])
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="+", default=[100, 4096, 65536])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    eng = Engine(0)
    rec = {"tool": "tools/dispatch_upcoming.py", "reps": args.reps, "sizes": []}
    for R in args.entries:
        rec["sizes"].append(run_size(eng, R, args.nodes, args.reps, args.k))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
