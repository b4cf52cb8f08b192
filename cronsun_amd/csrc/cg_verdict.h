// cg_verdict.h -- fire verdicts: where a fire of the unit walks (cg_admit.h,
// cg_lock.h) lies in the rule-major CSR of cg_expand_device, shared by
// k_admit_verdicts / k_lock_verdicts (cg_verdict.hip) and the host-side
// algorithm check in tests/native/verdict_host.cpp.
//
// The count chain leaves per (rule, plan segment) a run {anchor, count,
// daymask} and, after the scan, the output position run_off of its first fire.
// A fire t of rule r lies in the run of the segment (a, b] with a < t <= b,
// at the run's offset plus its rank inside the run: the closed form of
// cg_profile.h for closed-form and @every runs, a binary search of the run's
// own stretch of `times` for walked runs (which have no closed form).
#pragma once
#include "cg_profile.h"

namespace cg {

// bits of a verdict byte (include/cronsun_gpu.h: CG_VERDICT_*)
constexpr uint8_t kVerdictDropped = 1, kVerdictSkipped = 2;

// Index in `times` of fire t of the rule whose run records (anchor, count,
// dmask, off at stride 1) are given; t must be a fire of the rule's expansion
// over (t0, t1].  The caller checks times[result] == t: for an instant that is
// no fire the result is some index of the run's stretch (or -1: no run there).
CG_HD int64_t fire_position(const DSpec& sp, const Segment* segs, int G, const int64_t* anchor,
                            const int32_t* count, const uint32_t* dmask, const int64_t* off,
                            const int64_t* times, int64_t t1, int64_t t) {
  const int s = seg_after(segs, G, t - 1);
  if (s >= G) return -1;
  const int32_t n = count[s];
  if (n <= 0) return -1;
  const uint32_t dm = dmask[s];
  if (run_has_closed_form(sp, segs[s], dm)) {
    const CFRule c = cf_rule(sp);
    return off[s] + run_fires_upto(sp, c, segs[s], anchor[s], n, dm, t1, t) - 1;
  }
  // walked run: its fires are times[off[s] .. off[s] + n), ascending
  int64_t lo = off[s], hi = off[s] + n - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (times[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace cg
