#!/usr/bin/env python3
"""Measure the top-rules calls (cg_profile_top_rules_nodes /
cg_profile_top_rules_bucket) against the only route there was before them:
copy the whole rule matrix to the host (cg_profile_copy_rules), rebuild the
nodes' rule lists from cg_rule_nodes, and gather + lexsort per node in numpy.
No ratio is set in advance.

  config3  1M jobs x 10k nodes x 24 h, B = 24 one-hour buckets, the start and
           the in-flight profile: every node at its peak bucket, k = 10 and 64.
  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the cluster-wide
           row at one bucket, k = 64.

The results of the two routes are compared first.  Both then run in this
process, alternating, --pairs times each after two warm-ups; times are wall ms
around calls that end in a stream synchronise (the device route includes its
copy of the lists to the host).  The record carries cg_profile_top_rules_times
(device ms of the select and of the merge, the chunk count), the algorithmic
bytes of the pass -- per (row, rule) pair 4 bytes of rule index and one 4-byte
cell, plus (2k + 3) * 4 per row -- and what fraction of the HBM peak that is
over the select's device time.  One JSON line per shape goes to --out.

Run by hand on an MI355X:
    python tools/top_rules_bench.py --out profiles/top_rules_bench.json
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

HBM_PEAK = 8.0e12  # bytes/s, the part's specification


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
    """int64 [R] ms, log-uniform over [1 ms, 2 h] (as inflight_bench.py)."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(0.0, np.log(7_200_000.0), R)).astype(np.int64).clip(1, 7_200_000)


def upload(eng, R, seed):
    arr, status = cron.parse_batch(synth.spec_mix(R, seed=seed, mix=synth.MIX_CONFIG2), threads=16)
    assert (status == 0).all()
    return eng.upload_c(arr, R)


def host_top(matrix, off, rule, buckets, k):
    """The five columns from a host copy of the rule matrix and node-major
    lists: gather, drop the zero cells, lexsort by (-count, rule), cut."""
    N = len(off) - 1
    out_r = np.full((N, k), -1, dtype=np.int32)
    out_c = np.zeros((N, k), dtype=np.int32)
    nl, nc = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for n in range(N):
        r = rule[off[n]:off[n + 1]]
        c = matrix[r, buckets[n]]
        keep = c > 0
        r, c = r[keep], c[keep]
        order = np.lexsort((r, -c.astype(np.int64)))[:k]
        m = len(order)
        out_r[n, :m], out_c[n, :m] = r[order], c[order]
        nl[n], nc[n] = m, len(r)
    return out_r, out_c, nl, nc, np.asarray(buckets, dtype=np.int32)


def host_nodes_route(eng, rin, mode, k):
    """What a caller had to do before: the whole rule matrix and the peaks to
    the host, the join from cg_rule_nodes turned node-major, numpy per node."""
    matrix = eng.profile_rules()
    _, at = eng.profile_node_peaks()
    rn_off, rn_nodes = eng.rule_nodes(rin, mode)
    pair_rule = np.repeat(np.arange(rin.n_rules, dtype=np.int32), np.diff(rn_off))
    order = np.argsort(rn_nodes, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(rn_nodes, minlength=rin.n_nodes))]).astype(np.int64)
    return host_top(matrix, off, pair_rule[order], at, k)


def same(got, exp, what):
    for name, g, e in zip(("rule", "count", "n_listed", "n_contrib", "bucket"), got, exp):
        assert np.array_equal(g, e), f"{what}: {name} differs between the two routes"


def record(eng, pairs_nnz, rows, k, new_s, old_s):
    sel, merge, chunks = eng.profile_top_rules_ms()
    gathered = pairs_nnz * 4 + pairs_nnz * 4
    stored = rows * (2 * k + 3) * 4
    return {"k": k, "pairs": len(new_s["all"]), "warmups": 2, "order": "alternating, device route first in even pairs",
            "device_route_ms": new_s, "host_route_ms": old_s,
            "host_over_device_median": old_s["median"] / new_s["median"],
            "select_device_ms": sel, "merge_device_ms": merge, "chunks": int(chunks),
            "algorithmic_bytes": {"rule_indices": pairs_nnz * 4, "cells_gathered": pairs_nnz * 4, "result": stored},
            "select_fraction_of_hbm_peak": (gathered + stored) / (sel * 1e-3) / HBM_PEAK if sel > 0 else None}


def measure(args, sync, new, old):
    for _ in range(2):
        new()
        old()
    a, b = alternate(new, old, args.pairs, sync)
    new()  # so that cg_profile_top_rules_times is the device route's
    return stats(a), stats(b)


def config3(eng, torch, args):
    R, w, B, t0, N = args.rules, 3600, 24, synth.T0_2026, 10_000
    utc = cron.UTC()
    sp = upload(eng, R, 0x5EED + 3)
    rin = synth.rules_for_nodes(R, n_nodes=N, n_groups=500, seed=0x5EED + 3)
    dr = eng.upload_rules(rin)
    mode = _lib.EXCLUDE_NONE
    dur = durations(R, args.seed + 3)
    sync = torch.cuda.synchronize
    out = []
    for kind in ("starts", "inflight"):
        if kind == "starts":
            eng.profile_per_node(sp, utc, t0, w, B, dr, mode)
        else:
            eng.inflight_per_node(sp, utc, t0, w, B, dur, dr, mode)
        nnz = len(eng.rule_nodes(rin, mode)[1])
        for k in (10, 64):
            got = eng.profile_top_rules(k)
            same(got, host_nodes_route(eng, rin, mode, k), f"config3 {kind} k={k}")
            new_s, old_s = measure(args, sync, lambda: eng.profile_top_rules(k),
                                   lambda: host_nodes_route(eng, rin, mode, k))
            rec = {"shape": "config3 every node at its peak bucket", "profile": kind, "rules": R, "nodes": N,
                   "width_s": w, "buckets": B, "node_rule_pairs": nnz, "rows_compared": "all five columns: equal",
                   "contributors_max": int(got[3].max()), "rule_matrix_bytes_copied_by_host_route": R * B * 4}
            rec.update(record(eng, nnz, N, k, new_s, old_s))
            out.append(rec)
    dr.free()
    sp.free()
    return out


def config2(eng, torch, args):
    R, w, B, t0, k = args.rules, 60, 1440, synth.T0_2026, 64
    utc = cron.UTC()
    sp = upload(eng, R, 0x5EED)
    eng.profile_device(sp, utc, t0, w, B)
    bucket = 9 * 60  # 09:00-09:01, where hourly and daily rules fire
    off = np.array([0, R], dtype=np.int64)
    all_rules = np.arange(R, dtype=np.int32)

    def host():
        return host_top(eng.profile_rules(), off, all_rules, [bucket], k)
    got = eng.profile_top_rules_bucket(bucket, k)
    same(got, host(), "config2 cluster-wide")
    new_s, old_s = measure(args, torch.cuda.synchronize, lambda: eng.profile_top_rules_bucket(bucket, k), host)
    rec = {"shape": "config2 cluster-wide row, one bucket", "profile": "starts", "rules": R, "width_s": w,
           "buckets": B, "bucket": bucket, "rows_compared": "all five columns: equal",
           "contributors": int(got[3][0]), "rule_matrix_bytes_copied_by_host_route": R * B * 4}
    rec.update(record(eng, R, 1, k, new_s, old_s))
    rec["algorithmic_bytes"]["rule_indices"] = 0  # the row's rules are 0..R-1: no list is read
    sel = rec["select_device_ms"]
    rec["select_fraction_of_hbm_peak"] = (R * 4 + (2 * k + 3) * 4) / (sel * 1e-3) / HBM_PEAK if sel > 0 else None
    sp.free()
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_rules_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0xD0)
    ap.add_argument("--shapes", default="config3,config2")
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("at least five pairs")
    import torch
    eng = Engine(0)
    lines = []
    for name in args.shapes.split(","):
        for rec in {"config2": config2, "config3": config3}[name](eng, torch, args):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # kept after every shape
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    eng.close()


if __name__ == "__main__":
    main()
