#!/usr/bin/env python3
"""Measure the lock profile (cg_lock_profile_device / _per_node_device, kind
GRANTED) against the start profile of the same shape on the same box -- the
chain it extends by two kernels; no ratio is set in advance.

  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the rule matrix.
  config3  1M rules on 10 000 nodes, B = 24 one-hour buckets: the node matrix.

Every rule is its own unit.  Kinds are drawn from a seed, COMMON | ALONE |
INTERVAL at 0.6 | 0.2 | 0.2, AvgTime log-uniform from 1 ms to 2 h.  Before
anything is timed the results are held to the definition on the device:
granted + skipped is the start profile cell by cell, all COMMON grants every
fire, nobody contending grants every fire, the totals are the column sums, no
cell is negative, and every @every INTERVAL rule (a one-rule unit) skips
nothing.  Both calls run in this process, alternating, --pairs times each
after two warm-ups; times are wall ms around calls that end in a stream
synchronise, the kernels are timed by HIP events on the engine's stream
(cg_last_kernel_times [14..16], [19], [21]).  The record names the longest lane
of k_lock_units (the rule with the most granted fires: a lane steps once per
granted fire and asks Next twice there).

Run by hand on an MI355X:
    python tools/lock_bench.py --out profiles/lock_bench.json
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

START_KERNELS = ("k_profile_rules", "k_profile_walk", "k_profile_totals")
LOCK_KERNELS = START_KERNELS + ("k_admit_prepare", "k_lock_units")
SHARES = (0.6, 0.2, 0.2)


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


def draw(R, seed):
    """(kind int32 [R] in {COMMON, ALONE, INTERVAL}, avg_ms int64 [R] log-uniform over [1 ms, 2 h])."""
    rng = np.random.default_rng(seed)
    avg = np.exp(rng.uniform(0.0, np.log(7_200_000.0), R)).astype(np.int64).clip(1, 7_200_000)
    kind = rng.choice(np.array([_lib.JOB_COMMON, _lib.JOB_ALONE, _lib.JOB_INTERVAL], dtype=np.int32), R, p=SHARES)
    return kind, avg


def upload(eng, R, seed):
    specs = synth.spec_mix(R, seed=seed, mix=synth.MIX_CONFIG2)
    arr, status = cron.parse_batch(specs, threads=16)
    assert (status == 0).all()
    return specs, eng.upload_c(arr, R)


def identities(torch, call, starts, specs, kind, avg):
    """call(kind, contends, what) -> (rules, totals) views; starts: a copy of
    the start matrix.  Returns (granted rows' sums per rule, fires skipped)."""
    R = len(specs)
    rules, _ = call(np.zeros(R, dtype=np.int32), None, "granted")
    assert torch.equal(rules, starts), "all COMMON does not grant every fire"
    rules, totals = call(kind, np.zeros(R, dtype=np.uint8), "skipped")
    assert not bool(rules.any()) and not bool(totals.any()), "a rule that reaches no lock is skipped"
    skipped = call(kind, None, "skipped")[0].clone()
    rules, totals = call(kind, None, "granted")
    assert torch.equal(rules + skipped, starts), "granted + skipped is not the start profile"
    assert bool((rules >= 0).all()) and bool((skipped >= 0).all())
    assert torch.equal(totals, rules.sum(dim=0, dtype=torch.int64))
    every_interval = np.array([s.startswith("@every") for s in specs]) & (kind == _lib.JOB_INTERVAL)
    idx = torch.as_tensor(np.nonzero(every_interval)[0], device=skipped.device)
    assert not bool(skipped[idx].any()), "a one-rule @every INTERVAL unit skipped a fire"
    granted_per_rule = rules.sum(dim=1, dtype=torch.int64).cpu().numpy()
    return granted_per_rule, int(skipped.sum()), int(every_interval.sum())


def measure(eng, torch, pairs, new, old):
    sync = torch.cuda.synchronize
    for _ in range(2):  # warm-ups
        new()
        old()
    sync()
    new()
    kt_new = eng.profile_kernel_times() + eng.lock_kernel_times()
    old()
    kt_old = eng.profile_kernel_times()
    a, b = alternate(new, old, pairs, sync)
    return stats(a), stats(b), kt_new, kt_old


def record(shape, args, specs, kind, avg, granted_per_rule, n_starts, n_skipped, n_every, new_s, old_s, kt_new, kt_old,
           extra):
    lock = kind != _lib.JOB_COMMON
    lane = int(np.argmax(np.where(lock, granted_per_rule, -1)))
    rec = {"shape": shape, "rules": len(specs), "seed": args.seed, "units": "every rule its own unit",
           "kind_shares_common_alone_interval": list(SHARES), "avg_time_ms": "log-uniform 1 .. 7 200 000",
           "lock_ttl": 300, "lock_units": int(lock.sum()), "fires": n_starts, "fires_skipped": n_skipped,
           "every_interval_rules_checked": n_every,
           "longest_lane": {"rule": lane, "spec": specs[lane], "granted_fires": int(granted_per_rule[lane]),
                            "kind": int(kind[lane]), "avg_time_ms": int(avg[lane])},
           "identities": "granted + skipped = starts, all COMMON and nobody contending grant all, @every INTERVAL "
                         "never skips, totals = column sums, no negative cell: exact",
           "pairs": args.pairs, "warmups": 2, "order": "alternating, granted first in even pairs",
           "granted_ms": new_s, "start_profile_ms": old_s,
           "granted_kernels_ms": dict(zip(START_KERNELS + ("join", "node_matrix") + LOCK_KERNELS[3:], kt_new)),
           "start_profile_kernels_ms": dict(zip(START_KERNELS + ("join", "node_matrix"), kt_old)),
           "granted_minus_start_median_ms": new_s["median"] - old_s["median"],
           "start_profile_spread_ms": old_s["max"] - old_s["min"]}
    rec.update(extra)
    return rec


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    utc = cron.UTC()
    specs, sp = upload(eng, R, 0x5EED)
    kind, avg = draw(R, args.seed)
    call = lambda k, c, what: eng.lock_runs_device(sp, utc, t0, w, B, k, avg, None, c, 300, what)  # noqa: E731
    starts = eng.profile_device(sp, utc, t0, w, B)[0].clone()
    n_starts = int(starts.sum())
    gpr, n_skipped, n_every = identities(torch, call, starts, specs, kind, avg)
    del starts
    torch.cuda.empty_cache()
    new_s, old_s, kt_new, kt_old = measure(eng, torch, args.pairs, lambda: call(kind, None, "granted"),
                                           lambda: eng.profile_device(sp, utc, t0, w, B))
    rec = record("config2 rule matrix", args, specs, kind, avg, gpr, n_starts, n_skipped, n_every, new_s, old_s, kt_new,
                 kt_old, {"width_s": w, "buckets": B})
    sp.free()
    return rec


def config3(eng, torch, args):
    R, w, B, t0, N = args.rules, 3600, 24, synth.T0_2026, 10_000
    utc = cron.UTC()
    specs, sp = upload(eng, R, 0x5EED + 3)
    rin = synth.rules_for_nodes(R, n_nodes=N, n_groups=500, seed=0x5EED + 3)
    dr = eng.upload_rules(rin)
    mode = _lib.EXCLUDE_NONE
    kind, avg = draw(R, args.seed + 3)
    contends = eng.rule_contends(rin, mode)

    def call(k, c, what):
        rules, totals, nodes = eng.lock_runs_per_node_device(sp, utc, t0, w, B, k, avg, None, c, dr, mode, 300, what)
        call.nodes = nodes
        return rules, totals
    starts, _, start_nodes = [x.clone() for x in eng.profile_per_node_device(sp, utc, t0, w, B, dr, mode)]
    n_starts = int(starts.sum())
    gpr, n_skipped, n_every = identities(torch, call, starts, specs, kind, avg)
    call(np.zeros(R, dtype=np.int32), None, "granted")
    assert torch.equal(call.nodes, start_nodes), "node matrix of all COMMON"
    del starts, start_nodes
    torch.cuda.empty_cache()
    new_s, old_s, kt_new, kt_old = measure(eng, torch, args.pairs, lambda: call(kind, contends, "granted"),
                                           lambda: eng.profile_per_node_device(sp, utc, t0, w, B, dr, mode))
    rec = record("config3 node matrix", args, specs, kind, avg, gpr, n_starts, n_skipped, n_every, new_s, old_s, kt_new,
                 kt_old, {"width_s": w, "buckets": B, "nodes": N, "rules_that_contend": int(contends.sum())})
    dr.free()
    sp.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lock_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0x10C)
    ap.add_argument("--shapes", default="config2,config3")
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("at least five pairs")
    import torch
    eng = Engine(0)
    recs = []
    for name in args.shapes.split(","):
        recs.append({"config2": config2, "config3": config3}[name](eng, torch, args))
        print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
