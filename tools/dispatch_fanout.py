#!/usr/bin/env python3
"""Measure the dispatcher's node fan-out (cg_dispatcher_fanout) on the bench's
dispatch workload: synth.spec_mix entries (the 1M config-2 set, tiled past 1M
as bench.py does) bound to synth.rules_for_nodes over 10k nodes.

Three wakes per table size: the top of an hour (the densest), a top of a
minute, and the median (by due count) of a run of one-second wakes.  Each wake
reports the cg_dispatcher_fire time, the fan-out time with each path forced and
with AUTO (min / median / max over --reps repetitions of the same wake), n_due,
the pair total, nnz, the filter path's achieved bytes/s against
nnz * 4 + pairs * 4, and the crossover factor the wake suggests:
(due-driven time per pair) / (filter time per join pair).

Run by hand on an MI355X:
    python tools/dispatch_fanout.py --out profiles/dispatch_fanout.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cronsun_amd import _lib, cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402

PATHS = (("filter", _lib.CG_FANOUT_FILTER), ("due", _lib.CG_FANOUT_DUE), ("auto", _lib.CG_FANOUT_AUTO))


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def measure_fanout(eng, d, reps):
    """The last wake fanned out with each path, reps times: device ms (events
    around the fan-out, the pair-total read-back included) and wall ms."""
    out = {}
    pairs = None
    for name, path in PATHS:
        d.set_fanout_path(path)
        d.fanout_count()  # sizes the buffers
        dev, wall = [], []
        for _ in range(reps):
            t = time.perf_counter()
            n = d.fanout_count()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(eng.fanout_ms())
        assert pairs in (None, n)
        pairs = n
        out[name] = {"device_ms": spread(dev), "wall_ms": spread(wall)}
    d.set_fanout_path(_lib.CG_FANOUT_AUTO)
    return pairs, out


def wake_record(eng, d, now, reps, nnz):
    t = time.perf_counter()
    n_due, _ = d.fire_count(now)
    fire_wall = (time.perf_counter() - t) * 1e3
    kt = eng.dispatch_kernel_times()
    pairs, fan = measure_fanout(eng, d, reps)
    rec = {"now": int(now), "n_due": int(n_due), "pairs": int(pairs), "nnz": int(nnz),
           "fire_ms": {"scan": kt[0], "compact": kt[1], "advance": kt[2], "device_total": sum(kt),
                       "wall": fire_wall},
           "fanout": fan}
    f_ms = fan["filter"]["device_ms"]["min"]
    rec["filter_bytes"] = int(nnz * 4 + pairs * 4)
    rec["filter_gbps"] = rec["filter_bytes"] / (f_ms * 1e-3) / 1e9 if f_ms > 0 else None
    d_ms = fan["due"]["device_ms"]["min"]
    if pairs > 0 and f_ms > 0:
        rec["crossover_factor"] = (d_ms / pairs) / (f_ms / nnz)
    best = min(f_ms, d_ms)
    a = fan["auto"]["device_ms"]
    # AUTO against the better forced path, within the run-to-run spread of the wake
    sp = max(v["device_ms"]["max"] - v["device_ms"]["min"] for v in fan.values())
    rec["auto_vs_best_ms"] = a["min"] - best
    rec["spread_ms"] = sp
    rec["auto_ok"] = bool(a["min"] - best <= sp)
    return rec


def run_size(eng, R, n_nodes, reps, seconds):
    utc = cron.UTC()
    base = synth.spec_mix(min(R, 1_000_000), seed=0x5EED + 5, mix=synth.MIX_CONFIG2)
    specs = (base * (R // len(base) + 1))[:R]
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    sp = eng.upload_c(arr, R)
    rin = synth.rules_for_nodes(R, n_nodes=n_nodes, n_groups=500, seed=0x5EED + 3)
    drules = eng.upload_rules(rin)
    hour = synth.T0_2026 + 10 * 3600
    minute = hour + 17 * 60
    # (rule, node) pairs of the join: the count-only form of cg_rule_nodes
    c_rin, c_nnz = rin.to_c(), C.c_int64()
    _lib.check(_lib.lib().cg_rule_nodes(eng._h, C.byref(c_rin), _lib.EXCLUDE_NONE, None, None, 0, C.byref(c_nnz)))
    nnz = c_nnz.value
    out = {"entries": R, "nodes": n_nodes, "nnz": nnz, "wakes": {}}
    for name, T in (("top_of_hour", hour), ("top_of_minute", minute), ("one_second", minute + 20)):
        d = eng.dispatcher(sp, utc, T - 1)
        t = time.perf_counter()
        d.bind_rules(drules, _lib.EXCLUDE_NONE)
        bind_ms = (time.perf_counter() - t) * 1e3
        assert d.effective == T, (name, d.effective, T)  # the mix holds every-second entries
        if name != "one_second":
            rec = wake_record(eng, d, T, reps, nnz)
        else:
            recs = [wake_record(eng, d, T + s, reps, nnz) for s in range(seconds)]
            recs.sort(key=lambda r: r["n_due"])
            rec = recs[len(recs) // 2]
            rec["n_due_range"] = [recs[0]["n_due"], recs[-1]["n_due"]]
        rec["bind_ms"] = bind_ms
        out["wakes"][name] = rec
        d.free()
    drules.free()
    sp.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entries", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=int, default=21, help="one-second wakes the median is taken over")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    eng = Engine(0)
    rec = {"tool": "tools/dispatch_fanout.py", "reps": args.reps, "sizes": []}
    for R in args.entries:
        rec["sizes"].append(run_size(eng, R, args.nodes, args.reps, args.seconds))
        print(json.dumps(rec["sizes"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
