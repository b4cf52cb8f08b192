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

--patch measures cg_dispatcher_patch_rules instead, against a rebind of the
same edited set on the same dispatcher in the same run (alternating, --reps
times each): the node / group lists of 1000 random jobs, of one job, and the
membership of the group most rules reference.  A patch is timed as
upload_rules(patch) + patch_rules, a rebind as upload_rules(whole edited set)
+ bind_rules: wall ms around calls that end in a stream synchronise, and for
the patch the device ms of its phases (cg_dispatcher_patch_times).  The
fan-out of one dense wake after the patch must checksum equal to the one after
the rebind.

Run by hand on an MI355X:
    python tools/dispatch_fanout.py --out profiles/dispatch_fanout.json
    python tools/dispatch_fanout.py --patch --out profiles/dispatch_patch.json
"""
import argparse
import ctypes as C
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


PATCH_PHASES = ("patch_join", "rule_major_rows", "delta_pairs_sort", "removed_pairs_sort", "merge")


def cut_rules(rin, idx):
    """The rules idx (one job each, as synth.rules_for_nodes makes them) as
    their own rule set over the same nodes and groups."""
    from cronsun_amd.engine import RulesIn
    idx = np.asarray(idx, dtype=np.int64)

    def gather(off, vals):
        n = off[idx + 1] - off[idx]
        o = np.zeros(len(idx) + 1, dtype=np.int64)
        o[1:] = np.cumsum(n)
        src = np.repeat(off[idx] - o[:-1], n) + np.arange(int(o[-1]), dtype=np.int64)
        return o, vals[src]
    assert (rin.rule_job[idx] == idx).all()
    nid_off, nids = gather(rin.nid_off, rin.nids)
    gid_off, gids = gather(rin.gid_off, rin.gids)
    ex_off, ex = gather(rin.ex_off, rin.ex)
    return RulesIn(rin.n_nodes, rin.n_groups, len(idx), len(idx), group_off=rin.group_off,
                   group_nodes=rin.group_nodes, group_exists=rin.group_exists,
                   rule_job=np.arange(len(idx), dtype=np.int32), nid_off=nid_off, nids=nids,
                   gid_off=gid_off, gids=gids, ex_off=ex_off, ex=ex, job_pause=rin.job_pause[idx])


def relist_jobs(rin, idx, rng):
    """New random node / group / exclude lists (the same lengths) for rules idx, in place."""
    for off, vals, lim in ((rin.nid_off, rin.nids, rin.n_nodes), (rin.gid_off, rin.gids, rin.n_groups),
                           (rin.ex_off, rin.ex, rin.n_nodes)):
        for r in idx:
            a, b = int(off[r]), int(off[r + 1])
            vals[a:b] = rng.integers(0, lim, b - a)


def fanout_sums(eng, d):
    n = d.fanout_count()
    p_off, p_slots, _ = d.fanout_device()
    return n, eng.checksum(p_off, d._n_nodes + 1, 8), eng.checksum(p_slots, n, 4) if n else 0


def patch_record(eng, d, rin, idx, reps, what):
    """Patch of rules idx of the (already edited) set rin against a rebind of
    rin, alternating on d."""
    prin = cut_rules(rin, idx)
    slots = np.asarray(idx, dtype=np.int64)
    nnz_before = d_nnz(eng, rin)  # the edited set's join size (what both end at)
    for _ in range(2):  # warm-up in the order that is timed: both halves of the join sized
        dr = eng.upload_rules(prin)
        d.patch_rules(dr, slots)
        dr.free()
        sums_patch = fanout_sums(eng, d)
        df = eng.upload_rules(rin)
        d.bind_rules(df, _lib.EXCLUDE_NONE)
        df.free()
    up, pt, dev, phases, rup, rb = [], [], [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        dr = eng.upload_rules(prin)
        t1 = time.perf_counter()
        d.patch_rules(dr, slots)
        t2 = time.perf_counter()
        dr.free()
        ph = d.patch_ms()
        up.append((t1 - t) * 1e3)
        pt.append((t2 - t1) * 1e3)
        dev.append(sum(ph))
        phases.append(ph)
        t = time.perf_counter()
        df = eng.upload_rules(rin)
        t1 = time.perf_counter()
        d.bind_rules(df, _lib.EXCLUDE_NONE)
        t2 = time.perf_counter()
        df.free()
        rup.append((t1 - t) * 1e3)
        rb.append((t2 - t1) * 1e3)
    sums_bind = fanout_sums(eng, d)
    print("  %s: done" % what, file=sys.stderr, flush=True)
    wall = [a + b for a, b in zip(up, pt)]
    rwall = [a + b for a, b in zip(rup, rb)]
    nnz = nnz_before
    moved = 16 * nnz  # every pair read and written once on the rule-major and on the node-major side
    best = min(range(reps), key=lambda i: dev[i])
    return {"what": what, "patch_rules": int(len(idx)), "nnz": int(nnz),
            "patch": {"upload_wall_ms": spread(up), "patch_rules_wall_ms": spread(pt), "wall_ms": spread(wall),
                      "device_ms": spread(dev),
                      "phase_ms_of_fastest": dict(zip(PATCH_PHASES, phases[best]))},
            "rebind": {"upload_wall_ms": spread(rup), "bind_rules_wall_ms": spread(rb), "wall_ms": spread(rwall)},
            "bytes_streamed_16nnz": int(moved),
            "streamed_gbps_of_fastest": moved / (dev[best] * 1e-3) / 1e9 if dev[best] > 0 else None,
            "slowest_patch_vs_fastest_rebind_wall": max(wall) / min(rwall),
            "slowest_patch_rules_vs_fastest_bind_rules_wall": max(pt) / min(rb),
            "patch_faster": bool(max(wall) < min(rwall)),
            "fanout_pairs": int(sums_patch[0]), "fanout_matches_rebind": bool(sums_patch == sums_bind)}


def d_nnz(eng, rin):
    c_rin, c_nnz = rin.to_c(), C.c_int64()
    _lib.check(_lib.lib().cg_rule_nodes(eng._h, C.byref(c_rin), _lib.EXCLUDE_NONE, None, None, 0, C.byref(c_nnz)))
    return c_nnz.value


def run_patch_size(eng, R, n_nodes, reps):
    utc = cron.UTC()
    base = synth.spec_mix(min(R, 1_000_000), seed=0x5EED + 5, mix=synth.MIX_CONFIG2)
    specs = (base * (R // len(base) + 1))[:R]
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    sp = eng.upload_c(arr, R)
    rin = synth.rules_for_nodes(R, n_nodes=n_nodes, n_groups=500, seed=0x5EED + 3)
    hour = synth.T0_2026 + 10 * 3600
    d = eng.dispatcher(sp, utc, hour - 1)
    drules = eng.upload_rules(rin)
    d.bind_rules(drules, _lib.EXCLUDE_NONE)
    drules.free()
    d.fire_count(hour)  # the densest wake: its fan-out is compared after patch and rebind
    rng = np.random.default_rng(0x5EED + 9)
    out = {"entries": R, "nodes": n_nodes, "cases": []}
    idx = np.sort(rng.choice(R, 1000, replace=False))
    relist_jobs(rin, idx, rng)
    out["cases"].append(patch_record(eng, d, rin, idx, reps, "lists of 1000 random jobs"))
    idx = np.array([int(rng.integers(0, R))])
    relist_jobs(rin, idx, rng)
    out["cases"].append(patch_record(eng, d, rin, idx, reps, "lists of one job"))
    G = rin.n_groups
    refs = np.bincount(rin.gids[:rin.gid_off[R]], minlength=G)
    g = int(np.argmax(refs))
    a, b = int(rin.group_off[g]), int(rin.group_off[g + 1])
    rin.group_nodes[a:b] = rng.choice(n_nodes, b - a, replace=False)
    rule_of = np.repeat(np.arange(R, dtype=np.int64), np.diff(rin.gid_off[:R + 1]))
    idx = np.unique(rule_of[rin.gids[:rin.gid_off[R]] == g])
    out["cases"].append(patch_record(eng, d, rin, idx, reps,
                                     "membership of group %d (%d nodes), referenced by %d rules" % (g, b - a, len(idx))))
    d.free()
    sp.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entries", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seconds", type=int, default=21, help="one-second wakes the median is taken over")
    ap.add_argument("--out", default="")
    ap.add_argument("--patch", action="store_true", help="measure cg_dispatcher_patch_rules against a rebind")
    args = ap.parse_args()
    eng = Engine(0)
    if args.patch:
        rec = {"tool": "tools/dispatch_fanout.py --patch", "reps": args.reps, "sizes": []}
        for R in args.entries:
            rec["sizes"].append(run_patch_size(eng, R, args.nodes, args.reps))
            print(json.dumps(rec["sizes"][-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
        return
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
