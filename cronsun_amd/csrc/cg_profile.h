// cg_profile.h -- fire profile: bucketed fire counts per rule and per node
// without the fire lists (cg_profile.hip).  The closed form shared by the
// kernel and the host-side algorithm check in tests/native: how many fires of
// one run record lie at or before an instant.
//
// The count chain leaves, per (rule, plan segment), a run {anchor, count,
// daymask} (cg_expand.h, count_rule).  All fires of the run of segment (a, b]
// lie in (a, min(b, T1)], so the fires of a rule in a bucket (lo, hi] are the
// sum, over the segments the bucket overlaps, of
//   run_fires_upto(min(hi, b)) - run_fires_upto(max(lo, a)).
#pragma once
#include "cg_expand.h"

namespace cg {

// Fires of the run {anchor, count, dmask} of segment sg that are <= e, in
// [0, count].  e is clipped to the segment's end and t1.  Closed-form and
// @every runs only: a walked run (run_is_walked, and the rule not @every) has
// no closed form and is binned fire by fire (k_profile_walk).
CG_HD int32_t run_fires_upto(const DSpec& sp, const CFRule& c, const Segment& sg, int64_t anchor,
                             int32_t count, uint32_t dmask, int64_t t1, int64_t e) {
  if (count <= 0) return 0;
  int64_t end = sg.b < t1 ? sg.b : t1;
  if (e > end) e = end;
  int64_t n;
  if (sp.kind == KIND_EVERY) {
    // fires anchor + k*D, k = 1..count (constantdelay.go:25-27)
    if (e <= anchor) return 0;
    n = (e - anchor) / (int64_t)sp.sec;
  } else {
    // the anchor is the run's first fire
    if (e < anchor) return 0;
    n = 1 + cf_count(c, sg, dmask, anchor, e);
  }
  return (int32_t)(n < count ? n : count);
}

// a run the closed form above covers (else: walked fire by fire)
CG_HD bool run_has_closed_form(const DSpec& sp, const Segment& sg, uint32_t dmask) {
  return sp.kind == KIND_EVERY || !run_is_walked(sg, dmask);
}

// first segment whose end lies after instant x (G when none): the segment
// holding the first possible fire after x.  Binary search over the ends.
CG_HD int seg_after(const Segment* segs, int G, int64_t x) {
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (segs[mid].b > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Fires of one rule in bucket (lo, hi] from its closed-form runs (run records
// at stride 1 from the given pointers): walked runs contribute nothing here.
CG_HD int32_t profile_cell(const DSpec& sp, const CFRule& c, const Segment* segs, int G,
                           const int64_t* anchor, const int32_t* count, const uint32_t* dmask,
                           int64_t t1, int64_t lo, int64_t hi) {
  int32_t n = 0;
  for (int s = seg_after(segs, G, lo); s < G && segs[s].a < hi; s++) {
    const int32_t cnt = count[s];
    if (cnt == 0) continue;
    const uint32_t dm = dmask[s];
    if (!run_has_closed_form(sp, segs[s], dm)) continue;
    const int64_t a = anchor[s];
    const int64_t from = lo > segs[s].a ? lo : segs[s].a;
    n += run_fires_upto(sp, c, segs[s], a, cnt, dm, t1, hi) - run_fires_upto(sp, c, segs[s], a, cnt, dm, t1, from);
  }
  return n;
}

}  // namespace cg
