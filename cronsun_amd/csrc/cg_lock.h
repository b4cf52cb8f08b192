// cg_lock.h -- lock profile: which fires of a KindAlone / KindInterval job the
// etcd lock of Cmd.Run would let run and which it would skip (job.go:134-147,
// 194-271, client.go:95-109), shared by k_lock_units (cg_profile.hip) and the
// host-side algorithm check in tests/native/lock_host.cpp.
//
// A lock unit is a contiguous rule range [r0, r0 + k) -- the rules of one job,
// cluster-wide: the lock key is the job's ID -- of kind ALONE or INTERVAL.  The
// fires of its contending rules over (t0, t1], taken in order of (time, rule
// index), are granted while the key is gone (t >= free_at), else skipped.  A
// granted fire at t takes ttl = lock_ttl_of(Next(t), Next(Next(t)), ...) and
// holds the key until t + ttl (INTERVAL: no keep-alive) or until ttl seconds
// after the command ends, t + d + ttl (ALONE: kept alive while it runs).  The
// walk below never visits the fires a held key skips.
#pragma once
#include "cg_admit.h"

namespace cg {

// one lock unit with a contending rule, as the host compacts them for the kernel
struct LockUnit {
  int64_t r0;      // first rule
  int64_t avg_ms;  // Job.AvgTime as stored (may be negative: lock_ttl_of)
  int64_t d;       // ceil(max(avg_ms, 0) / 1000), clamped to the horizon
  int32_t k;       // rules
  int32_t kind;    // JOB_ALONE or JOB_INTERVAL
};

// LDS bytes of one lane's walk cache (cg_admit.h, AdmitWalkCache): there is no ring
constexpr size_t kLockLaneBytes = size_t(kAdmitWalkSlots) * (8 + 3 * 4);

// what the host check counts (null in the kernel)
struct LockWalkStats {
  long long jumps = 0;      // skip-ahead steps over a held key
  long long ttl_evals = 0;  // fires that found the key gone
  long long ttl_past = 0;   // ... whose Next(Next(t)) lay past t1
  long long ttl_zero = 0;   // ... whose ttl was 0 (skipped, state unchanged)
};

// The granted fires of one lock unit, in order: emit(rule, time) for each.
// admit_walk_unit's position (t, q) and admit_fire_after over the contending
// rules (contends[r] != 0; null: all); no cursor per rule.  While t < free_at
// every fire is skipped: the position moves to (free_at - 1, last rule) in one
// step.  A fire that finds the key gone costs two Next calls past any horizon
// (next_exact with bound INT64_MAX over the zone table, which must reach as
// far as cg_lock_ttl_batch's; @every D: x + D), not read off the run records.
// Returns -1, or the rule whose Next never returns (CG_NO_PROGRESS): the
// reference hangs there, and the rows are then unfinished.
template <class Emit>
CG_HD int64_t lock_walk_unit(const DSpec* specs, const ZoneView& z, const Segment* segs, int G,
                             const int64_t* run_anchor, const int32_t* run_count, const uint32_t* run_dmask,
                             int64_t t0, int64_t t1, const LockUnit& u, int64_t lock_ttl, const uint8_t* contends,
                             const AdmitWalkCache& wc, Emit&& emit, LockWalkStats* stats = nullptr) {
  const int64_t r1 = u.r0 + u.k;
  int64_t t = t0, q = r1 - 1;
  int64_t free_at = INT64_MIN;
  for (int i = 0; i < kAdmitWalkSlots; i++) wc.rel[i * wc.stride] = -1;
  for (;;) {
    int64_t bt = INT64_MAX, br = -1;
    for (int64_t r = u.r0; r < r1; r++) {
      if (contends && !contends[r]) continue;
      const DSpec sp = specs[r];
      const int64_t j0 = r * G;
      const int64_t e = admit_fire_after(sp, z, segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, t0, t1,
                                         r > q ? t - 1 : t, int32_t(r - u.r0), wc);
      if (e < bt) {  // the lower rule wins a second
        bt = e;
        br = r;
      }
    }
    if (br < 0) return -1;
    t = bt;
    q = br;
    if (t < free_at) {  // the key exists: so it does for every fire before free_at
      t = free_at - 1;
      q = r1 - 1;
      if (stats) stats->jumps++;
      continue;
    }
    // Cmd.lockTtl at now = t (k_lock_ttl's arithmetic): a = Next(t), b = Next(a)
    const DSpec sp = specs[q];
    int64_t a = t, b = t;
#ifdef __clang__
#pragma unroll 1  // one inlined copy of next_exact
#endif
    for (int i = 0; i < 2; i++) {
      a = b;
      b = sp.kind == KIND_EVERY ? b + int64_t(sp.sec) : next_exact(sp, z, b, INT64_MAX);
      if (b == CG_NO_PROGRESS) break;
    }
    const int64_t ttl = lock_ttl_of(a, b, u.kind, u.avg_ms, lock_ttl);
    if (ttl == CG_NO_PROGRESS) return q;
    if (stats) {
      stats->ttl_evals++;
      if (b > t1) stats->ttl_past++;
      if (ttl == 0) stats->ttl_zero++;
    }
    if (ttl == 0) continue;  // lock() returns nil (job.go:246-248): skipped, the key untouched
    emit(q, t);
    // ttl < 2^54 whatever lock_ttl is (a saturated Sub less an AvgTime / 1000): no overflow
    free_at = t + (u.kind == JOB_ALONE ? u.d : 0) + ttl;
  }
}

}  // namespace cg
