#!/usr/bin/env python3
"""Measure the running profile (kind RUNNING of cg_admit_*, LOCK_RUNNING of
cg_lock_profile_*) against the ADMITTED / GRANTED call of the same shape on the
same box -- the chain it changes in three places: in-flight base rows instead
of start rows, a second read-modify-write per started fire, and k_rows_prefix.
No ratio is set in advance.

  config2  1M mixed rules x 24 h, B = 1440 one-minute buckets: the rule matrix.
  config3  1M rules on 10 000 nodes, B = 24 one-hour buckets: the node matrix.

Workloads, mixes and seeds are tools/admit_bench.py's (admission flavour) and
tools/lock_bench.py's (lock flavour); every rule is its own unit.  Before
anything is timed the results are held to the definition on the device:
running <= in flight cell by cell; no limit (all COMMON) gives the in-flight
profile; 0 ms gives zero; the totals are the column sums; and the rules whose
run time is one bucket wide have their ADMITTED / GRANTED rows.  Both calls
run in this process, alternating, --pairs times each after two warm-ups; times
are wall ms around calls that end in a stream synchronise, the kernels are
timed by HIP events on the engine's stream (cg_last_kernel_times [14], [15],
[19], [20] / [21], [22]).  k_rows_prefix's algorithmic bytes are rewritten
rows x B x 8 (each cell read and stored once).  Zones with walked runs at this
size are not measured.

Run by hand on an MI355X:
    python tools/running_bench.py --out profiles/running_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import admit_bench  # noqa: E402
import lock_bench  # noqa: E402
from cronsun_amd import _lib, cron, synth  # noqa: E402
from cronsun_amd.engine import Engine  # noqa: E402

SLOTS = {14: "rule_matrix", 15: "walked_runs", 16: "k_profile_totals", 19: "k_admit_prepare", 20: "k_admit_units",
         21: "k_lock_units", 22: "k_rows_prefix"}
PEAK_BYTES_PER_S = 8e12


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


def slots(eng):
    buf = (C.c_float * 23)()
    _lib.check(_lib.lib().cg_last_kernel_times(eng._h, buf, 23))
    return {name: buf[i] for i, name in SLOTS.items()}


def measure(eng, torch, pairs, new, old):
    sync = torch.cuda.synchronize
    for _ in range(2):  # warm-ups
        new()
        old()
    sync()
    new()
    kt_new = slots(eng)
    old()
    kt_old = slots(eng)
    a, b = alternate(new, old, pairs, sync)
    return stats(a), stats(b), kt_new, kt_old


def record(shape, flavour, base, R, B, rewritten, n_run, n_infl, new_s, old_s, kt_new, kt_old, extra):
    bytes_ = rewritten * B * 8
    ms = kt_new["k_rows_prefix"]
    rec = {"shape": shape, "flavour": flavour, "rules": R, "buckets": B, "units": "every rule its own unit",
           "rewritten_rows": rewritten, "running_cells_sum": n_run, "inflight_cells_sum": n_infl,
           "identities": "running <= in flight, no limit = in flight, 0 ms = zero, one-bucket run times = the "
                         f"{base} rows, totals = column sums: exact",
           "pairs": len(new_s["all"]), "warmups": 2, "order": "alternating, running first in even pairs",
           "running_ms": new_s, f"{base}_ms": old_s,
           "running_kernels_ms": kt_new, f"{base}_kernels_ms": kt_old,
           f"running_minus_{base}_median_ms": new_s["median"] - old_s["median"],
           f"{base}_spread_ms": old_s["max"] - old_s["min"],
           "where_ms": {"k_rows_prefix": ms,
                        "base_rows_minus_start_rows": (kt_new["rule_matrix"] + kt_new["walked_runs"]) -
                                                      (kt_old["rule_matrix"] + kt_old["walked_runs"]),
                        "unit_walk_second_store": (kt_new["k_admit_units"] + kt_new["k_lock_units"]) -
                                                  (kt_old["k_admit_units"] + kt_old["k_lock_units"])},
           "k_rows_prefix_algorithmic_bytes": bytes_,
           "k_rows_prefix_bytes_per_s": bytes_ / (ms * 1e-3) if ms > 0 else None,
           "k_rows_prefix_share_of_8TBps": bytes_ / (ms * 1e-3) / PEAK_BYTES_PER_S if ms > 0 else None}
    rec.update(extra)
    return rec


def one_bucket_rows(torch, run, starts, dur_ms, w):
    idx = np.nonzero((dur_ms > (w - 1) * 1000) & (dur_ms <= w * 1000))[0]
    i = torch.as_tensor(idx, device=run.device)
    assert torch.equal(run[i], starts[i]), "a rule running one bucket width does not have its start rows"
    return int(idx.size)


# ------------------------------------------------------------ admission --
def admission(eng, torch, args, shape, sp, R, w, B, t0, seed, dr=None, mode=0):
    utc = cron.UTC()
    shares = [float(x) for x in args.parallels_shares.split(",")]
    dur, par = admit_bench.draw(R, seed, shares)
    zeros = np.zeros(R, dtype=np.int64)
    L, z = _lib.lib(), eng._loc(utc).handle

    def call(d, p, what):
        d, p, _, k = eng._admit_args(R, d, p, None, what)
        if dr is None:
            _lib.check(L.cg_admit_device(eng._h, sp._h, z, t0, w, B, d.ctypes.data, p.ctypes.data, None, k))
        else:
            _lib.check(L.cg_admit_per_node_device(eng._h, sp._h, z, t0, w, B, d.ctypes.data, p.ctypes.data, None, k,
                                                  dr._h, mode))
        return eng._profile_tensors()
    infl = eng.inflight_device(sp, utc, t0, w, B, dur)[0].clone()
    out = call(dur, zeros, "running")
    assert torch.equal(out[0], infl), "no limit is not the in-flight profile"
    out = call(zeros, par, "running")
    assert not bool(out[0].any()) and not bool(out[1].any()), "0 ms runs"
    adm = call(dur, par, "admitted")[0].clone()
    out = call(dur, par, "running")
    run = out[0]
    assert bool((run <= infl).all()) and bool((run >= 0).all()), "running exceeds in flight"
    assert torch.equal(out[1], run.sum(dim=0, dtype=torch.int64))
    n_one = one_bucket_rows(torch, run, adm, dur, w)
    if dr is not None:
        assert bool((out[2] >= 0).all())
    d_sec = np.minimum(dur // 1000 + (dur % 1000 != 0), w * B)
    could = (par > 0) & (d_sec > par)
    n_run, n_infl = int(run.sum()), int(infl.sum())
    del infl, adm, run, out
    torch.cuda.empty_cache()
    new_s, old_s, kt_new, kt_old = measure(eng, torch, args.pairs, lambda: call(dur, par, "running"),
                                           lambda: call(dur, par, "admitted"))
    return record(shape, "admission", "admitted", R, B, int(could.sum()), n_run, n_infl, new_s, old_s, kt_new, kt_old,
                  {"width_s": w, "seed": seed, "parallels_shares_0_1_2": shares, "one_bucket_rules_checked": n_one})


# ------------------------------------------------------------------ lock --
def lock(eng, torch, args, shape, sp, R, w, B, t0, seed, dr=None, mode=0, contends=None):
    utc = cron.UTC()
    kind, avg = lock_bench.draw(R, seed)
    L, z = _lib.lib(), eng._loc(utc).handle

    def call(k, what):
        k, a, _, c, ttl, wh = eng._lock_args(R, k, avg, None, contends, 300, what)
        cp = None if c is None else c.ctypes.data
        if dr is None:
            _lib.check(L.cg_lock_profile_device(eng._h, sp._h, z, t0, w, B, k.ctypes.data, a.ctypes.data, None, cp,
                                                ttl, wh))
        else:
            _lib.check(L.cg_lock_profile_per_node_device(eng._h, sp._h, z, t0, w, B, k.ctypes.data, a.ctypes.data, None,
                                                         cp, ttl, wh, dr._h, mode))
        return eng._profile_tensors()
    infl = eng.inflight_device(sp, utc, t0, w, B, avg)[0].clone()
    out = call(np.zeros(R, dtype=np.int32), "running")
    assert torch.equal(out[0], infl), "all COMMON is not the in-flight profile"
    granted = call(kind, "granted")[0].clone()
    out = call(kind, "running")
    run = out[0]
    assert bool((run <= infl).all()) and bool((run >= 0).all()), "running exceeds in flight"
    assert torch.equal(out[1], run.sum(dim=0, dtype=torch.int64))
    n_one = one_bucket_rows(torch, run, granted, avg, w)
    locked = (kind != _lib.JOB_COMMON) & (np.ones(R, bool) if contends is None else contends != 0)
    n_run, n_infl = int(run.sum()), int(infl.sum())
    del infl, granted, run, out
    torch.cuda.empty_cache()
    new_s, old_s, kt_new, kt_old = measure(eng, torch, args.pairs, lambda: call(kind, "running"),
                                           lambda: call(kind, "granted"))
    return record(shape, "lock", "granted", R, B, int(locked.sum()), n_run, n_infl, new_s, old_s, kt_new, kt_old,
                  {"width_s": w, "seed": seed, "kind_shares_common_alone_interval": list(lock_bench.SHARES),
                   "lock_ttl": 300, "one_bucket_rules_checked": n_one})


def config2(eng, torch, args):
    R, w, B, t0 = args.rules, 60, 1440, synth.T0_2026
    _, sp = lock_bench.upload(eng, R, 0x5EED)
    recs = [admission(eng, torch, args, "config2 rule matrix", sp, R, w, B, t0, args.admit_seed),
            lock(eng, torch, args, "config2 rule matrix", sp, R, w, B, t0, args.lock_seed)]
    sp.free()
    return recs


def config3(eng, torch, args):
    R, w, B, t0, N = args.rules, 3600, 24, synth.T0_2026, 10_000
    _, sp = lock_bench.upload(eng, R, 0x5EED + 3)
    rin = synth.rules_for_nodes(R, n_nodes=N, n_groups=500, seed=0x5EED + 3)
    dr = eng.upload_rules(rin)
    mode = _lib.EXCLUDE_NONE
    contends = eng.rule_contends(rin, mode)
    recs = [admission(eng, torch, args, "config3 node matrix", sp, R, w, B, t0, args.admit_seed + 3, dr, mode),
            lock(eng, torch, args, "config3 node matrix", sp, R, w, B, t0, args.lock_seed + 3, dr, mode, contends)]
    for r in recs:
        r["nodes"] = N
    dr.free()
    sp.free()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "running_bench.json"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rules", type=int, default=1_000_000)
    ap.add_argument("--admit-seed", type=int, default=0xAD)
    ap.add_argument("--lock-seed", type=int, default=0x10C)
    ap.add_argument("--parallels-shares", default="0.5,0.3,0.2", help="shares of Parallels 0, 1 and 2")
    ap.add_argument("--shapes", default="config2,config3")
    args = ap.parse_args()
    if args.pairs < 5:
        ap.error("at least five pairs")
    import torch
    eng = Engine(0)
    recs = []
    for name in args.shapes.split(","):
        for rec in {"config2": config2, "config3": config3}[name](eng, torch, args):
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
