// cg_admit.h -- admission profile: which fires of a job Job.limit() would let
// run and which it would drop (job.go:134-139, 165-187), shared by
// k_admit_units (cg_profile.hip) and the host-side algorithm check in
// tests/native/admit_host.cpp.
//
// A unit is a contiguous rule range [r0, r0 + k) -- the rules of one job on
// one node -- with a limit P >= 1 and an expected run time of d >= 1 whole
// seconds.  Its fires over (t0, t1], taken in order of (time, rule index), are
// admitted while fewer than P admitted fires a of the unit have a + d > t,
// else dropped.  The walk below never visits the fires a saturated unit drops.
#pragma once
#include "cg_profile.h"

namespace cg {

// largest limit of a unit that can still drop (the ring of admitted starts);
// include/cronsun_gpu.h: CG_ADMIT_MAX_PARALLELS
constexpr int kAdmitMaxParallels = 16;

// one unit that can drop, as the host compacts them for the kernel
struct AdmitUnit {
  int64_t r0;  // first rule
  int64_t d;   // whole seconds, >= 1, clamped to the horizon
  int32_t k;   // rules
  int32_t P;   // 1..kAdmitMaxParallels
};

// A unit with no limit, no run time, or a limit its k rules cannot reach (at
// most one fire per rule and second, so at most k * d started and unfinished)
// never drops: its rows are the start profile's.
CG_HD bool admit_never_drops(int64_t P, int64_t d, int64_t k) { return P == 0 || d == 0 || d <= P / k; }

// Remembered positions inside walked runs, kAdmitWalkSlots of them per unit:
// slot (rule - r0) % kAdmitWalkSlots holds, for one rule, its run s and the
// last fire t of that run at or before the instant last asked for (q fires
// stepped to reach it).  A later question about the same run at a later
// instant resumes there, so a unit of up to kAdmitWalkSlots rules steps each
// walked fire once, as k_profile_walk does; rules that share a slot evict
// each other and step again from the run's anchor -- slower, never wrong.
// Slot i of a field lies at [i * stride] (LDS in the kernel, one column per
// lane; no dynamic index into registers).
constexpr int kAdmitWalkSlots = 8;
struct AdmitWalkCache {
  int64_t* t;
  int32_t *rel, *s, *q;
  int stride;
};
// LDS bytes of one lane's ring and walk cache
constexpr size_t kAdmitLaneBytes = size_t(kAdmitMaxParallels) * 8 + size_t(kAdmitWalkSlots) * (8 + 3 * 4);

// First fire of rule r's expansion over (t0, t1] that lies after instant x, or
// INT64_MAX: read off the run records (anchor/count/dmask at stride 1), so it
// is the start profile's expansion by construction -- Next_r(x) of a fire x,
// and for any other x the fire the reference's loop from t0 reaches next.
// (Calling Next on an arbitrary instant is not that near a zone transition.)
//   @every D      t0 + (floor((x - t0) / D) + 1) * D: anchored at t0
//   closed form   the run's anchor when x lies before it, else the first
//                 matching local time after x inside the segment
//   walked run    stepped by next_exact from the run's anchor (or from the
//                 rule's remembered position; rel = rule - first rule of the unit)
CG_HD int64_t admit_fire_after(const DSpec& sp, const ZoneView& z, const Segment* segs, int G,
                               const int64_t* anchor, const int32_t* count, const uint32_t* dmask, int64_t t0,
                               int64_t t1, int64_t x, int32_t rel, const AdmitWalkCache& wc) {
  if (x < t0) x = t0;
  if (x >= t1) return INT64_MAX;
  if (sp.kind == KIND_EVERY) {
    const int64_t D = (int64_t)sp.sec;
    const int64_t e = t0 + ((x - t0) / D + 1) * D;
    return e <= t1 ? e : INT64_MAX;
  }
  const CFRule c = cf_rule(sp);
  for (int s = seg_after(segs, G, x); s < G && segs[s].a < t1; s++) {
    const int32_t n = count[s];
    if (n == 0) continue;
    const uint32_t dm = dmask[s];
    if (!run_is_walked(segs[s], dm)) {
      if (x < anchor[s]) return anchor[s];
      const int64_t b = segs[s].b < t1 ? segs[s].b : t1;
      const int64_t e = cf_first_after(c, segs[s], dm, x);
      if (e <= b) return e;
      continue;
    }
    int64_t t = anchor[s];
    int32_t q = 0;
    const int slot = (rel % kAdmitWalkSlots) * wc.stride;
    if (wc.rel[slot] == rel && wc.s[slot] == s && wc.t[slot] <= x) {
      t = wc.t[slot];
      q = wc.q[slot];
    }
    while (q < n) {
      const int64_t e = next_exact(sp, z, t, t1);
      if (e > x) {
        wc.rel[slot] = rel;
        wc.s[slot] = s;
        wc.q[slot] = q;
        wc.t[slot] = t;
        return e;
      }
      t = e;
      q++;
    }
  }
  return INT64_MAX;
}

// The admitted fires of one unit, in order: emit(rule, time) for each.
// Position (t, q) is the last fire processed; the next one is the least
// (time, rule) among the rules' first fires after t - 1 (rules above q) or
// after t (rules up to q) -- no cursor is kept per rule, so a unit may hold
// any number of rules.  ring holds the last P admitted starts at
// ring[i * stride] (LDS in the kernel, one column per lane), wc the walked
// runs' remembered positions.  When the ring is full and its oldest entry a'
// is still running at t, every fire before F = a' + d is dropped: the position
// moves to (F - 1, last rule) in one step.
template <class Emit>
CG_HD void admit_walk_unit(const DSpec* specs, const ZoneView& z, const Segment* segs, int G,
                           const int64_t* run_anchor, const int32_t* run_count, const uint32_t* run_dmask,
                           int64_t t0, int64_t t1, const AdmitUnit& u, int64_t* ring, int stride,
                           const AdmitWalkCache& wc, Emit&& emit) {
  const int64_t r1 = u.r0 + u.k;
  int64_t t = t0, q = r1 - 1;
  int32_t head = 0, held = 0;
  for (int i = 0; i < kAdmitWalkSlots; i++) wc.rel[i * wc.stride] = -1;
  for (;;) {
    int64_t bt = INT64_MAX, br = -1;
    for (int64_t r = u.r0; r < r1; r++) {
      const DSpec sp = specs[r];
      const int64_t j0 = r * G;
      const int64_t e = admit_fire_after(sp, z, segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, t0, t1,
                                         r > q ? t - 1 : t, int32_t(r - u.r0), wc);
      if (e < bt) {  // the lower rule wins a second
        bt = e;
        br = r;
      }
    }
    if (br < 0) return;
    t = bt;
    q = br;
    if (held == u.P) {
      const int64_t F = ring[head * stride] + u.d;
      if (F > t) {
        t = F - 1;
        q = r1 - 1;
        continue;
      }
      ring[head * stride] = t;
      head = head + 1 == u.P ? 0 : head + 1;
    } else {
      ring[held * stride] = t;
      held++;
    }
    emit(q, t);
  }
}

}  // namespace cg
