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

// ------------------------------------------------------- in-flight profile --
// Commands of one rule running at bucket edge e = t0 + (b+1)*w, given an
// expected run time of d whole seconds (the job's AvgTime in ms, rounded up):
// the fires t of the rule's expansion over (t0, t1] with e - d < t <= e.
// Fire times are whole seconds, so that is "started at or before e and not
// yet finished at e" (t <= e < t + ms/1000) -- hence the rounding up.  (This
// is not Cmd.lockTtl's `cost`, job.go:213-221, which rounds AvgTime down.)
// Commands started at or before t0 are unknown and not counted: the lower
// edge is clipped to t0, and a row ramps up over its first d seconds.  The
// caller clamps d to t1 - t0, so e - d cannot overflow.

// seconds of a duration in ms, rounded up and clamped to the horizon
inline int64_t inflight_seconds(int64_t dur_ms, int64_t horizon) {
  const int64_t d = dur_ms / 1000 + (dur_ms % 1000 != 0);
  return d < horizon ? d : horizon;
}

// the closed-form runs' share of the cell at edge e (walked runs: below)
CG_HD int32_t inflight_cell(const DSpec& sp, const CFRule& c, const Segment* segs, int G,
                            const int64_t* anchor, const int32_t* count, const uint32_t* dmask,
                            int64_t t0, int64_t t1, int64_t e, int64_t d) {
  const int64_t lo = e - d > t0 ? e - d : t0;
  return profile_cell(sp, c, segs, G, anchor, count, dmask, t1, lo, e);
}

// Cursor over the walked fires of one rule in ascending order (its walked
// runs in segment order, each stepped by next_exact from the run's anchor):
// t is the next fire not yet consumed, INT64_MAX past the last.
struct WalkCursor {
  int s = -1;            // run (segment) of t
  int32_t q = 0, n = 0;  // fires of run s stepped so far, and its count
  int64_t t = 0;
};

CG_HD void walk_cursor_next(WalkCursor& k, const DSpec& sp, const ZoneView& z, const Segment* segs, int G,
                            const int64_t* anchor, const int32_t* count, const uint32_t* dmask, int64_t t1) {
  while (k.s < G) {
    if (k.q < k.n) {
      k.q++;
      k.t = next_exact(sp, z, k.t, t1);
      return;
    }
    for (k.s++; k.s < G; k.s++)
      if (count[k.s] != 0 && run_is_walked(segs[k.s], dmask[k.s])) break;
    if (k.s < G) {
      k.q = 0;
      k.n = count[k.s];
      k.t = anchor[k.s];
    }
  }
  k.t = INT64_MAX;
}

// The walked runs' share of one rule's row, added to row [B].  A walked fire t
// is in flight at buckets (t - t0 - 1) / w .. (t + d - 1 - t0) / w - 1; adding
// 1 to each of them per fire would cost fires x buckets (an every-second rule
// in an hour-wide WALK window with a long d).  Instead the touched buckets are
// swept once with two cursors over the fires: at edge e the head has passed
// the fires <= e and the tail the fires <= e - d, and the cell gains head -
// tail.  Buckets in which nothing is in flight (between walked runs, beyond
// the last fire plus d) are skipped: O(fires + buckets touched).
CG_HD void inflight_walk_row(const DSpec& sp, const ZoneView& z, const Segment* segs, int G,
                             const int64_t* anchor, const int32_t* count, const uint32_t* dmask,
                             int64_t t0, int64_t t1, int64_t w, int32_t B, int64_t d, int32_t* row) {
  if (sp.kind == KIND_EVERY || d <= 0) return;  // closed form in every segment / never in flight
  WalkCursor head, tail;
  walk_cursor_next(head, sp, z, segs, G, anchor, count, dmask, t1);
  if (head.t == INT64_MAX) return;
  walk_cursor_next(tail, sp, z, segs, G, anchor, count, dmask, t1);
  int32_t nh = 0, nt = 0;
  int64_t b = head.t > t0 ? (head.t - t0 - 1) / w : 0;  // (fires lie in (t0, t1]: the row is never left)
  while (b < B) {
    const int64_t e = t0 + (b + 1) * w;
    while (head.t <= e) {
      nh++;
      walk_cursor_next(head, sp, z, segs, G, anchor, count, dmask, t1);
    }
    while (tail.t <= e - d) {
      nt++;
      walk_cursor_next(tail, sp, z, segs, G, anchor, count, dmask, t1);
    }
    row[b] += nh - nt;
    b++;
    if (nh == nt) {  // nothing in flight: on to the bucket of the next fire
      if (head.t == INT64_MAX) break;
      const int64_t nb = (head.t - t0 - 1) / w;
      if (nb > b) b = nb;
    }
  }
}

// -------------------------------------------------------- running profile --
// Commands in flight counting only the fires that start (the admitted fires of
// cg_admit.h, the granted ones of cg_lock.h).  A fire a in (t0, t1] with a run
// time of d whole seconds is in flight at the edges of buckets lo .. hi - 1
// (e_b - d < a <= e_b), the range inflight_walk_row names; hi may lie past B.
struct BucketRange {
  int64_t lo, hi;
};
CG_HD BucketRange running_range(int64_t a, int64_t d, int64_t t0, int64_t w) {
  return BucketRange{(a - t0 - 1) / w, (a + d - 1 - t0) / w};
}

// One started fire as a difference in the rule's own row: +1 where it comes
// into flight, -1 at the first bucket whose edge it no longer reaches (none
// when it runs past the last edge).  An inclusive prefix sum along the row
// (k_rows_prefix; the host check's loop) turns the differences into the cells,
// at 2 stores per fire rather than one per bucket it spans.  d == 0, or a run
// that ends before the next edge, leaves nothing.
CG_HD void running_emit_diff(int32_t* row, int32_t B, int64_t a, int64_t d, int64_t t0, int64_t w) {
  if (a <= t0) return;
  const BucketRange g = running_range(a, d, t0, w);
  if (g.hi == g.lo || g.lo >= B) return;
  row[g.lo] += 1;
  if (g.hi < B) row[g.hi] -= 1;
}

}  // namespace cg
