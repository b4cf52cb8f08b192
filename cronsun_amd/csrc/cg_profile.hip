// cg_profile.hip -- fire profile: fires per (rule, bucket) and per (node,
// bucket) over B fixed-width buckets of (t0, t0 + B*w], computed from the run
// records of the count chain and the cached rule->node transpose; no fire
// list is written ("load profile").
//
//   k_profile_rules   one lane per cell of the rule matrix [R][B], lanes along
//                     buckets: the closed-form runs' fires per bucket
//                     (cg_profile.h, profile_cell); every cell stored once
//   k_profile_walk    one lane per rule: the walked runs' fires, stepped by
//                     next_exact and added to the rule's own row
//   k_profile_totals  column sums of the rule matrix (int64 [B])
//   k_profile_nodes   node matrix [N][B] = transpose x rule matrix (integer
//                     SpMM): per (chunk of a node's rule list, 64-bucket tile)
//   k_profile_nodes_reduce  sums the chunk partials of nodes whose list spans
//                     more than one chunk
//
// In-flight profile (cg_inflight_*): commands running at each bucket edge,
// given a duration per rule.  The same chain with the first two kernels
// replaced; totals, node matrix and accessors are shared.
//   k_inflight_rules  k_profile_rules' mapping; cell = fires in (max(t0,
//                     e_b - d_r), e_b] (cg_profile.h, inflight_cell)
//   k_inflight_walk   one lane per rule: one two-cursor sweep over the buckets
//                     its walked fires touch (inflight_walk_row)
//   k_node_peaks      one wave per node row: (max cell, first bucket with it)
//
// Admission profile (cg_admit_*: the fires Job.limit() would admit, or those it
// would drop) and lock profile (cg_lock_profile_*: the fires the KindAlone /
// KindInterval lock of Cmd.Run would grant, or skip).  The start profile's
// first two kernels fill the rule matrix, then a unit walk rewrites rows
// (kernel side cg_unit_walk.h, host side cg_units.h); the rest is shared.
//   k_admit_prepare   one lane per cell: zeroes the flagged rows -- of units
//                     that can drop / contending rules of lock units -- when
//                     the kind counts up (ADMITTED, GRANTED), else the others
//   k_admit_units     one lane per unit that can drop: adds (ADMITTED) or
//                     subtracts (DROPPED) 1 per admitted fire in the rule's row
//   k_lock_units      one lane per lock unit with a contending rule: the same
//                     per granted fire (GRANTED / SKIPPED)
// Running profile (CG_PROFILE_RUNNING / CG_PROFILE_LOCK_RUNNING): commands in
// flight counting only the fires that start.  The in-flight chain's first two
// kernels, k_admit_prepare zeroing the flagged rows, the unit walk in
// difference mode (cg_profile.h, running_emit_diff), then
//   k_rows_prefix     in-place inclusive prefix sum along each flagged row
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_profile.h"
#include "cg_unit_walk.h"
#include "cg_units.h"

using namespace cg;

namespace {

constexpr int kMaxBuckets = 4096;
// rules of a node's list (k_profile_nodes: kNodeChunk, cg_api_internal.h) /
// rows of the rule matrix (k_profile_totals) summed by one block per bucket tile
constexpr int kTotalChunk = 4096;
static_assert(kAdmitMaxParallels == CG_ADMIT_MAX_PARALLELS, "cg_admit.h and the public header disagree");
static_assert(JOB_COMMON == CG_JOB_COMMON && JOB_ALONE == CG_JOB_ALONE && JOB_INTERVAL == CG_JOB_INTERVAL,
              "cg_time.h and the public header disagree");

// ------------------------------------------------------------ rule matrix --
__global__ __launch_bounds__(256) void k_profile_rules(const DSpec* __restrict__ specs, int64_t R, PlanArgs p,
                                                        const int64_t* __restrict__ run_anchor,
                                                        const int32_t* __restrict__ run_count,
                                                        const uint32_t* __restrict__ run_dmask, int64_t w, int32_t B,
                                                        int32_t* __restrict__ out) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  const int G = p.G;
  const int64_t cells = R * B, stride = int64_t(gridDim.x) * blockDim.x;
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= cells) return;
  // cell i = (rule r, bucket b), advanced without a division per cell
  const int64_t dr = stride / B;
  const int32_t db = int32_t(stride - dr * B);
  int64_t r = i / B;
  int32_t b = int32_t(i - r * B);
  for (; i < cells; i += stride) {
    const DSpec sp = load_spec(specs + r);
    const CFRule c = cf_rule(sp);
    const int64_t j0 = r * G;
    const int64_t lo = p.t0 + int64_t(b) * w;
    out[i] = profile_cell(sp, c, v.segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, p.t1, lo, lo + w);
    r += dr;
    b += db;
    if (b >= B) {
      b -= B;
      r++;
    }
  }
}

__global__ __launch_bounds__(256) void k_profile_walk(const DSpec* __restrict__ specs, int64_t R, PlanArgs p,
                                                       const int64_t* __restrict__ run_anchor,
                                                       const int32_t* __restrict__ run_count,
                                                       const uint32_t* __restrict__ run_dmask, int64_t w, int32_t B,
                                                       int32_t* __restrict__ out) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  const int G = p.G;
  for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < R; r += int64_t(gridDim.x) * blockDim.x) {
    DSpec sp;
    bool loaded = false;
    int32_t* row = out + r * B;  // this lane's own row
    for (int s = 0; s < G; s++) {
      const int64_t j = r * G + s;
      const int32_t n = run_count[j];
      if (n == 0 || !run_is_walked(v.segs[s], run_dmask[j])) continue;
      if (!loaded) {
        sp = load_spec(specs + r);
        loaded = true;
      }
      if (sp.kind == KIND_EVERY) break;  // closed form in every segment
      int64_t t = run_anchor[j];
      for (int32_t q = 0; q < n; q++) {
        t = next_exact(sp, v.z, t, p.t1);
        const int64_t b = (t - p.t0 - 1) / w;
        if (t > p.t0 && b < B) row[b] += 1;
      }
    }
  }
}

// ------------------------------------------------------ in-flight profile --
// k_profile_rules' lane mapping; cell (r, b) counts the fires in (max(t0,
// e - dsec[r]), e] at the bucket's upper edge e (cg_profile.h,
// inflight_cell).  dsec [R]: whole seconds, clamped to B * w by the host.
__global__ __launch_bounds__(256) void k_inflight_rules(const DSpec* __restrict__ specs, int64_t R, PlanArgs p,
                                                         const int64_t* __restrict__ run_anchor,
                                                         const int32_t* __restrict__ run_count,
                                                         const uint32_t* __restrict__ run_dmask,
                                                         const int64_t* __restrict__ dsec, int64_t w, int32_t B,
                                                         int32_t* __restrict__ out) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  const int G = p.G;
  const int64_t cells = R * B, stride = int64_t(gridDim.x) * blockDim.x;
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= cells) return;
  const int64_t dr = stride / B;
  const int32_t db = int32_t(stride - dr * B);
  int64_t r = i / B;
  int32_t b = int32_t(i - r * B);
  for (; i < cells; i += stride) {
    const DSpec sp = load_spec(specs + r);
    const CFRule c = cf_rule(sp);
    const int64_t j0 = r * G;
    out[i] = inflight_cell(sp, c, v.segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, p.t0, p.t1,
                           p.t0 + (int64_t(b) + 1) * w, dsec[r]);
    r += dr;
    b += db;
    if (b >= B) {
      b -= B;
      r++;
    }
  }
}

// one lane per rule: the walked runs' share, swept once over the touched
// buckets of the rule's own row (cg_profile.h, inflight_walk_row)
__global__ __launch_bounds__(256) void k_inflight_walk(const DSpec* __restrict__ specs, int64_t R, PlanArgs p,
                                                        const int64_t* __restrict__ run_anchor,
                                                        const int32_t* __restrict__ run_count,
                                                        const uint32_t* __restrict__ run_dmask,
                                                        const int64_t* __restrict__ dsec, int64_t w, int32_t B,
                                                        int32_t* __restrict__ out) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  const int G = p.G;
  for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < R; r += int64_t(gridDim.x) * blockDim.x) {
    const int64_t j0 = r * G;
    bool walked = false;
    for (int s = 0; s < G && !walked; s++) walked = run_count[j0 + s] != 0 && run_is_walked(v.segs[s], run_dmask[j0 + s]);
    if (!walked) continue;
    const DSpec sp = load_spec(specs + r);
    inflight_walk_row(sp, v.z, v.segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, p.t0, p.t1, w, B, dsec[r],
                      out + r * B);
  }
}

// ------------------------------------------------------ admission profile --
// Rows of the rule matrix a call of this kind rewrites: flag[r] != 0 marks the
// rules of units that can drop.  ADMITTED (zero_flagged): those rows restart
// from zero and k_admit_units counts the admitted fires into them; DROPPED:
// the rows of units that never drop are zero, the others keep their starts
// for k_admit_units to subtract from.  One lane per cell, 64-bit index.
__global__ __launch_bounds__(256) void k_admit_prepare(const uint8_t* __restrict__ flag, int64_t R, int32_t B,
                                                        int zero_flagged, int32_t* __restrict__ out) {
  const int64_t cells = R * B, stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < cells; i += stride)
    if ((flag[i / B] != 0) == (zero_flagged != 0)) out[i] = 0;
}

// A unit kernel's fire t of rule r (d: the unit's run time): `step` added to the
// cell of the rule's own row (a row belongs to one unit: plain read-modify-write)
// or, with diff != 0 (RUNNING kinds), the fire's difference over d
// (cg_profile.h, running_emit_diff; step is not read), which k_rows_prefix sums.
struct ProfileEmit {
  int64_t t0, w;
  int32_t B, step, diff;
  int32_t* out;
  __device__ __forceinline__ void operator()(int64_t r, int64_t t, int64_t d) const {
    if (diff) {
      running_emit_diff(out + r * B, B, t, d, t0, w);
      return;
    }
    const int64_t b = (t - t0 - 1) / w;
    if (t > t0 && b < B) out[r * B + b] += step;
  }
};

// One lane per unit that can drop (units [U], compacted by the host so waves are
// dense; cg_unit_walk.h).  step: +1 ADMITTED, -1 DROPPED (start - admitted).
__global__ __launch_bounds__(kUnitBlock) void k_admit_units(const DSpec* __restrict__ specs, PlanArgs p,
                                                             const int64_t* __restrict__ run_anchor,
                                                             const int32_t* __restrict__ run_count,
                                                             const uint32_t* __restrict__ run_dmask,
                                                             const AdmitUnit* __restrict__ units, int64_t U,
                                                             size_t ring_off, int64_t w, int32_t B, int32_t step,
                                                             int32_t diff, int32_t* __restrict__ out) {
  const ProfileEmit e{p.t0, w, B, step, diff, out};
  admit_unit_lane(specs, p, run_anchor, run_count, run_dmask, units, U, ring_off,
                  [&](const PlanView&, const AdmitUnit& u, int64_t r, int64_t t) { e(r, t, u.d); });
}

// ----------------------------------------------------------- lock profile --
// One lane per lock unit with a contending rule.  step: +1 GRANTED, -1 SKIPPED
// (start - granted); in difference mode the command runs u.d whatever its lease
// does.  contends [R]: the prepare pass's flags, inside a lock unit "this rule
// reaches the lock".  A rule whose Next never returns lowers *stuck to its index.
__global__ __launch_bounds__(kUnitBlock) void k_lock_units(const DSpec* __restrict__ specs, PlanArgs p,
                                                            const int64_t* __restrict__ run_anchor,
                                                            const int32_t* __restrict__ run_count,
                                                            const uint32_t* __restrict__ run_dmask,
                                                            const LockUnit* __restrict__ units, int64_t U,
                                                            const uint8_t* __restrict__ contends, size_t cache_off,
                                                            int64_t lock_ttl, int64_t w, int32_t B, int32_t step,
                                                            int32_t diff, int32_t* __restrict__ out,
                                                            unsigned long long* __restrict__ stuck) {
  const ProfileEmit e{p.t0, w, B, step, diff, out};
  const int64_t bad =
      lock_unit_lane(specs, p, run_anchor, run_count, run_dmask, units, U, cache_off, contends, lock_ttl,
                     [&](const PlanView&, const LockUnit& u, int64_t r, int64_t t) { e(r, t, u.d); });
  if (bad >= 0) atomicMin(stuck, static_cast<unsigned long long>(bad));
}

// one wave per row of the node matrix: (largest cell, first bucket attaining
// it).  Lanes stride the buckets in ascending order, so a lane keeps the first
// of equal cells; the wave reduction breaks ties to the smaller bucket.
__global__ __launch_bounds__(256) void k_node_peaks(const int64_t* __restrict__ nodes, int32_t N, int32_t B,
                                                     int64_t* __restrict__ peak, int32_t* __restrict__ bucket) {
  const int32_t lane = threadIdx.x & 63;
  const int64_t n = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (n >= N) return;  // a whole wave
  const int64_t* row = nodes + n * B;
  int64_t best = -1;  // cells are >= 0, and lane 0 always holds bucket 0
  int32_t at = 0x7FFFFFFF;
  for (int32_t b = lane; b < B; b += 64) {
    const int64_t x = row[b];
    if (x > best) {
      best = x;
      at = b;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const int32_t lo = __shfl_xor(int32_t(best), m, 64), hi = __shfl_xor(int32_t(best >> 32), m, 64);
    const int64_t ob = (int64_t(hi) << 32) | uint32_t(lo);
    const int32_t oa = __shfl_xor(at, m, 64);
    if (ob > best || (ob == best && oa < at)) {
      best = ob;
      at = oa;
    }
  }
  if (lane == 0) {
    peak[n] = best;
    bucket[n] = at;
  }
}

// ------------------------------------------------- column / node list sums --
// A block sums rows of the rule matrix for one tile of up to 64 buckets,
// lanes along buckets.  With B < 64 a wave holds 64 / B rows side by side, so
// a block works on `slots` rows at a time: row slot, bucket col of a thread.
struct TileLane {
  int32_t W, slots, slot, col;
  bool active;
};
__device__ __forceinline__ TileLane tile_lane(int32_t B) {
  TileLane t;
  t.W = B < 64 ? B : 64;
  const int32_t k = 64 / t.W, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int32_t sub = lane / t.W;
  t.col = int32_t(blockIdx.y) * 64 + (lane - sub * t.W);
  t.slots = 4 * k;
  t.slot = wv * k + sub;
  t.active = sub < k && t.col < B;
  return t;
}
// sum of the block's per-thread partials per bucket, valid in threads < W
__device__ __forceinline__ int64_t tile_reduce(const TileLane& t, int64_t acc) {
  __shared__ int64_t sh[256];
  sh[threadIdx.x] = t.active ? acc : 0;
  __syncthreads();
  int64_t sum = 0;
  if (int32_t(threadIdx.x) < t.W) {
    const int32_t k = t.slots / 4;
    for (int wv = 0; wv < 4; wv++)
      for (int s = 0; s < k; s++) sum += sh[wv * 64 + s * t.W + threadIdx.x];
  }
  return sum;
}

// tot [B] zeroed before the launch: one 64-bit atomic per block and column
__global__ __launch_bounds__(256) void k_profile_totals(const int32_t* __restrict__ rc, int64_t R, int32_t B,
                                                         unsigned long long* __restrict__ tot) {
  const TileLane t = tile_lane(B);
  const int64_t beg = int64_t(blockIdx.x) * kTotalChunk, end = beg + kTotalChunk < R ? beg + kTotalChunk : R;
  int64_t acc = 0;
  if (t.active) {
#pragma unroll 4
    for (int64_t r = beg + t.slot; r < end; r += t.slots) acc += rc[r * B + t.col];
  }
  const int64_t sum = tile_reduce(t, acc);
  if (int32_t(threadIdx.x) < t.W && t.col < B && sum != 0) atomicAdd(tot + t.col, (unsigned long long)sum);
}

// --------------------------------------------------------- running profile --
// Inclusive scan of x over the 64 lanes of the wave, by DPP (no LDS round
// trips): row_shr 1/2/4/8 inside each 16-lane row, row_bcast:15 adds the last
// lane of rows 0 and 2 to rows 1 and 3, row_bcast:31 lane 31 to rows 2 and 3.
// All 64 lanes must be active.
__device__ __forceinline__ int32_t scan_wave(int32_t x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2, 3
  return x;
}

// In-place inclusive prefix sum along the buckets of every flagged row of the
// rule matrix (flag [R]: the prepare pass's); other rows are neither read nor
// written.  Every cell is stored once by the one lane that owns it, so the
// result does not depend on the grid.  Rows are strided over the grid, 64-bit
// cell index.
//   B >= 64  one wave per row (the flag is wave-uniform: an unflagged row costs
//            one byte), 64-cell chunks loaded coalesced; the next chunk's load
//            is issued before the current chunk's scan, the carry is lane 63's
//            result of the previous chunk
//   B < 64   tile_lane's (slot, col): 64 / B rows side by side in a wave, a
//            Hillis-Steele scan in which a lane takes only from lanes of its
//            own slot (col >= offset); B need not be a power of two
__global__ __launch_bounds__(256) void k_rows_prefix(const uint8_t* __restrict__ flag, int64_t R, int32_t B,
                                                      int32_t* __restrict__ out) {
  if (B >= 64) {
    const int32_t lane = threadIdx.x & 63;
    for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < R; r += int64_t(gridDim.x) * 4) {
      if (!flag[r]) continue;  // a whole wave
      int32_t* row = out + r * B;
      int32_t carry = 0, next = row[lane];
      for (int32_t c0 = 0; c0 < B; c0 += 64) {
        const int32_t i = c0 + lane;
        int32_t x = next;
        next = i + 64 < B ? row[i + 64] : 0;
        x = scan_wave(x) + carry;  // lanes past B hold 0: lane 63 has the row's sum so far
        if (i < B) row[i] = x;
        carry = __builtin_amdgcn_readlane(x, 63);
      }
    }
    return;
  }
  const TileLane t = tile_lane(B);  // (gridDim.y == 1: col is the bucket)
  for (int64_t r0 = int64_t(blockIdx.x) * t.slots; r0 < R; r0 += int64_t(gridDim.x) * t.slots) {
    const int64_t r = r0 + t.slot;
    const bool mine = t.active && r < R && flag[r] != 0;
    int32_t x = mine ? out[r * B + t.col] : 0;
    for (int32_t o = 1; o < B; o <<= 1) {  // every lane shuffles; only its own slot's lanes feed it
      const int32_t y = __shfl_up(x, o, 64);
      if (t.col >= o) x += y;
    }
    if (mine) out[r * B + t.col] = x;
  }
}

// chunks of kNodeChunk rules a node's list is cut into (a node without rules
// still has one: its block stores the zero row)
__global__ void k_profile_chunks(const int64_t* __restrict__ nt_off, int32_t N, int32_t* __restrict__ cnt) {
  const int32_t n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int64_t len = nt_off[n + 1] - nt_off[n];
  cnt[n] = int32_t(len <= kNodeChunk ? 1 : (len + kNodeChunk - 1) / kNodeChunk);
}

// block (x, y): chunk x of the nodes' rule lists (chunk_off [N+1] = exclusive
// scan of the chunk counts), bucket tile y.  A single-chunk node's cells go
// straight to out, a heavy node's partial sums to part [chunk][B].
__global__ __launch_bounds__(256) void k_profile_nodes(const int64_t* __restrict__ nt_off,
                                                        const int32_t* __restrict__ nt_rule,
                                                        const int64_t* __restrict__ chunk_off, int32_t N,
                                                        const int32_t* __restrict__ rc, int32_t B,
                                                        int64_t* __restrict__ out, int64_t* __restrict__ part) {
  const int64_t ch = blockIdx.x;
  if (ch >= chunk_off[N]) return;
  // the node of chunk ch: the last n with chunk_off[n] <= ch
  int32_t n0 = 0, n1 = N - 1;
  while (n0 < n1) {
    const int32_t mid = (n0 + n1 + 1) >> 1;
    if (chunk_off[mid] <= ch) n0 = mid;
    else n1 = mid - 1;
  }
  const int32_t n = n0;
  const int64_t c0 = chunk_off[n], nch = chunk_off[n + 1] - c0;
  const int64_t beg = nt_off[n] + (ch - c0) * kNodeChunk;
  const int64_t lend = nt_off[n + 1], end = beg + kNodeChunk < lend ? beg + kNodeChunk : lend;
  const TileLane t = tile_lane(B);
  int64_t acc = 0;
  if (t.active) {
    // four independent (rule index, row) load pairs in flight per lane
    const int64_t step = t.slots;
    int64_t j = beg + t.slot;
    for (; j + 3 * step < end; j += 4 * step) {
      const int64_t r0 = nt_rule[j], r1 = nt_rule[j + step], r2 = nt_rule[j + 2 * step], r3 = nt_rule[j + 3 * step];
      const int32_t x0 = rc[r0 * B + t.col], x1 = rc[r1 * B + t.col], x2 = rc[r2 * B + t.col],
                    x3 = rc[r3 * B + t.col];
      acc += int64_t(x0) + x1 + x2 + x3;
    }
    for (; j < end; j += step) acc += rc[int64_t(nt_rule[j]) * B + t.col];
  }
  const int64_t sum = tile_reduce(t, acc);
  if (int32_t(threadIdx.x) < t.W && t.col < B) {
    if (nch == 1) out[int64_t(n) * B + t.col] = sum;
    else part[ch * B + t.col] = sum;
  }
}

// the cells of nodes with more than one chunk: the sum of their partials
__global__ __launch_bounds__(256) void k_profile_nodes_reduce(const int64_t* __restrict__ chunk_off, int32_t N,
                                                               int32_t B, const int64_t* __restrict__ part,
                                                               int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= int64_t(N) * B) return;
  const int64_t n = i / B;
  const int32_t col = int32_t(i - n * B);
  const int64_t c0 = chunk_off[n], c1 = chunk_off[n + 1];
  if (c1 - c0 <= 1) return;
  int64_t sum = 0;
  for (int64_t c = c0; c < c1; c++) sum += part[c * B + col];
  out[i] = sum;
}

// ------------------------------------------------------------------ host --
int profile_check_args(const char* what, const cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t width,
                       int32_t n_buckets) {
  if (!c || !s || !z) return cg_fail(CG_EINVAL, std::string(what) + ": null");
  if (n_buckets < 1 || n_buckets > kMaxBuckets)
    return cg_fail(CG_EINVAL, std::string(what) + ": n_buckets must be in [1, " + std::to_string(kMaxBuckets) + "]");
  if (width < 1) return cg_fail(CG_EINVAL, std::string(what) + ": width must be at least 1 second");
  if (width > CG_MAX_HORIZON / n_buckets)
    return cg_fail(CG_ERANGE, std::string(what) + ": n_buckets * width exceeds CG_MAX_HORIZON (40 years)");
  return CG_OK;
}

// What a profile call computes, built by its entry point: the kind, the
// in-flight durations (host, [R], whole seconds clamped to B * w; null: the base
// rows are the start profile's) and an admission or a lock call's checked
// arguments (cg_units.h; at most one).  A RUNNING kind has both.
struct ProfileCall {
  int kind = CG_PROFILE_STARTS;
  const std::vector<int64_t>* dsec = nullptr;
  const AdmitCall* adm = nullptr;
  const LockCall* lk = nullptr;
  static ProfileCall inflight(const std::vector<int64_t>* d) { return {CG_PROFILE_INFLIGHT, d, nullptr, nullptr}; }
  static ProfileCall admission(const AdmitCall* a) { return {a->what, a->durations(), a, nullptr}; }
  static ProfileCall lock(const LockCall* l) { return {l->what, l->durations(), nullptr, l}; }
  bool has_unit_walk() const { return adm || lk; }
  bool running() const { return kind == CG_PROFILE_RUNNING || kind == CG_PROFILE_LOCK_RUNNING; }
  int64_t units() const { return int64_t(adm ? adm->units.size() : lk ? lk->units.size() : 0); }
  // k_admit_prepare zeroes the flagged rows (else the others); the walk adds (else subtracts)
  bool counts_up() const { return kind != CG_PROFILE_DROPPED && kind != CG_PROFILE_LOCK_SKIPPED; }
};

// the event the unit walk ends at (every call records it, with or without a walk)
hipEvent_t walk_end_event(cg_ctx* c, bool running) { return c->pfev[running ? PFEV_PREFIX : PFEV_TOTALS]; }

// base rows: the start profile's or, with durations, the in-flight profile's
int profile_base_rows(cg_ctx* c, const cg_specs* s, int64_t w, int32_t B, const ProfileCall& pc) {
  RunSet& rs = c->rs;
  hipStream_t st = c->st;
  const int64_t R = int64_t(s->n);
  const size_t lds = plan_lds_bytes(rs.pa);
  if (pc.dsec) {
    // (*dsec outlives the stream synchronise that ends the call)
    if (int rc = c->pf_dur.ensure(size_t(R))) return rc;
    HIPCHK(hipMemcpyAsync(c->pf_dur.p, pc.dsec->data(), size_t(R) * 8, hipMemcpyHostToDevice, st));
  }
  // either flavour's kernel of a step: the in-flight one also takes the durations
  const auto launch = [&](auto starts, auto inflight, int blocks) {
    if (pc.dsec)
      hipLaunchKernelGGL(inflight, dim3(blocks), dim3(256), lds, st, s->d, R, rs.pa, rs.run_anchor.p, rs.run_count.p,
                         rs.run_dmask.p, c->pf_dur.p, w, B, c->pf_rules.p);
    else
      hipLaunchKernelGGL(starts, dim3(blocks), dim3(256), lds, st, s->d, R, rs.pa, rs.run_anchor.p, rs.run_count.p,
                         rs.run_dmask.p, w, B, c->pf_rules.p);
  };
  (void)hipEventRecord(c->pfev[PFEV_RULES], st);
  launch(k_profile_rules, k_inflight_rules, gridn(R * B, 256, 4096));
  (void)hipEventRecord(c->pfev[PFEV_WALK], st);
  if (rs.has_walk()) launch(k_profile_walk, k_inflight_walk, gridn(R, 256, 256 * 16));
  return CG_OK;
}

// the base rows are in place: an admission or a lock call rewrites them on the
// same stream.  A lock call then drains the stream to learn of a stuck rule.
int profile_unit_rewrite(cg_ctx* c, const cg_specs* s, int64_t w, int32_t B, const ProfileCall& pc) {
  RunSet& rs = c->rs;
  hipStream_t st = c->st;
  const int64_t R = int64_t(s->n), U = pc.units();
  const size_t lds = plan_lds_bytes(rs.pa), tail_off = unit_tail_off(lds);
  const int32_t step = pc.counts_up() ? 1 : -1, diff = pc.running() ? 1 : 0;
  const unsigned blocks = unsigned((U + kUnitBlock - 1) / kUnitBlock);
  if (int rc = unit_upload(c, R, pc.adm, pc.lk, nullptr, pc.lk != nullptr)) return rc;
  const uint8_t* flag = c->uw_flag[pc.lk ? 1 : 0].p;
  (void)hipEventRecord(c->pfev[PFEV_PREPARE], st);
  hipLaunchKernelGGL(k_admit_prepare, dim3(gridn(R * B, 256, 4096)), dim3(256), 0, st, flag, R, B,
                     pc.counts_up() ? 1 : 0, c->pf_rules.p);
  (void)hipEventRecord(c->pfev[PFEV_UNITS], st);
  if (U > 0 && pc.adm)
    hipLaunchKernelGGL(k_admit_units, dim3(blocks), dim3(kUnitBlock), admit_lds_bytes(lds), st, s->d, rs.pa,
                       rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, uw_admit_units(c), U, tail_off, w, B, step,
                       diff, c->pf_rules.p);
  if (U > 0 && pc.lk)
    hipLaunchKernelGGL(k_lock_units, dim3(blocks), dim3(kUnitBlock), lock_lds_bytes(lds), st, s->d, rs.pa,
                       rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, uw_lock_units(c), U, flag, tail_off,
                       pc.lk->lock_ttl, w, B, step, diff, c->pf_rules.p, c->uw_err.p + 1);
  (void)hipEventRecord(walk_end_event(c, pc.running()), st);
  if (!pc.lk) return CG_OK;
  HIPCHK(hipGetLastError());
  unsigned long long err[2];
  if (int rc = unit_errors(c, err)) return rc;
  if (err[1] != ~0ULL) return cg_fail(CG_ERANGE, lock_stuck_msg("cg_lock_profile", err[1]));  // no profile
  return CG_OK;
}

// a RUNNING call's flagged rows hold differences: summed along the buckets (no
// unit to walk: no row is flagged); then the column totals of any kind
int profile_prefix_totals(cg_ctx* c, int64_t R, int32_t B, const ProfileCall& pc) {
  hipStream_t st = c->st;
  if (pc.running()) {
    if (pc.units() > 0)
      hipLaunchKernelGGL(k_rows_prefix, dim3(gridn(R, B >= 64 ? 4 : 4 * (64 / B), 4096)), dim3(256), 0, st,
                         c->uw_flag[pc.lk ? 1 : 0].p, R, B, c->pf_rules.p);
    (void)hipEventRecord(c->pfev[PFEV_TOTALS], st);
  }
  hipLaunchKernelGGL(k_profile_totals, dim3(gridn(R, kTotalChunk, 1 << 30), (B + 63) / 64), dim3(256), 0, st,
                     c->pf_rules.p, R, B, reinterpret_cast<unsigned long long*>(c->pf_totals.p));
  (void)hipEventRecord(c->pfev[PFEV_TOTALS_END], st);
  HIPCHK(hipGetLastError());
  return CG_OK;
}

// count chain + rule matrix + totals, enqueued on the ctx stream (the caller drains it); c->mu
// held.  Every event is recorded once up front, so the slots of a phase that does not run read 0.
int profile_rules_enqueue(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t w, int32_t B,
                          const ProfileCall& pc) {
  c->pf_valid = false;
  c->pf_has_nodes = false;
  c->pf_peaks_valid = false;
  c->tr_valid = false;  // a top-rules result does not outlive its profile
  int rc;
  bool empty = true;
  if ((rc = sync_count_scan(c, s, z, t0, t0 + int64_t(B) * w, &empty, 0, pc.lk != nullptr))) return rc;
  if ((rc = ensure_events(c->pfev))) return rc;
  const int64_t R = int64_t(s->n);
  if ((rc = c->pf_rules.ensure(size_t(std::max<int64_t>(R * B, 1)))) || (rc = c->pf_totals.ensure(size_t(B))))
    return rc;
  hipStream_t st = c->st;
  HIPCHK(hipMemsetAsync(c->pf_totals.p, 0, size_t(B) * 8, st));
  for (int i = KT_PF_RULES; i < KT_COUNT; i++) c->kt[i] = 0.f;
  for (int i : {PFEV_RULES, PFEV_WALK, PFEV_PREPARE, PFEV_UNITS}) (void)hipEventRecord(c->pfev[i], st);
  if (pc.running()) (void)hipEventRecord(c->pfev[PFEV_PREFIX], st);
  for (int i : {PFEV_TOTALS, PFEV_TOTALS_END}) (void)hipEventRecord(c->pfev[i], st);
  if (!empty) {
    // a rule whose reference loop never ends: refuse before any cell is computed
    HIPCHK(hipStreamSynchronize(st));
    const unsigned long long stuck = static_cast<unsigned long long>(c->rs.res_host[1]);
    if (stuck != ~0ULL) return cg_fail(CG_ERANGE, stuck_msg(stuck));
    const size_t lds = plan_lds_bytes(c->rs.pa);
    if (pc.units() > 0 && (rc = pc.adm ? admit_lds_check("cg_admit", lds) : lock_lds_check("cg_lock_profile", lds)))
      return rc;
    if ((rc = profile_base_rows(c, s, w, B, pc))) return rc;
    if (pc.has_unit_walk()) {
      if ((rc = profile_unit_rewrite(c, s, w, B, pc))) return rc;
    } else {
      (void)hipEventRecord(walk_end_event(c, false), st);
    }
    if ((rc = profile_prefix_totals(c, R, B, pc))) return rc;
  }
  c->pf_R = R;
  c->pf_B = B;
  c->pf_N = 0;
  c->pf_kind = pc.kind;
  return CG_OK;
}

void profile_rule_times(cg_ctx* c) {
  const auto ms = [c](Kt slot, int from, hipEvent_t to) { (void)hipEventElapsedTime(&c->kt[slot], c->pfev[from], to); };
  const int k = c->pf_kind;
  const bool running = k == CG_PROFILE_RUNNING || k == CG_PROFILE_LOCK_RUNNING;
  const bool admission = k == CG_PROFILE_ADMITTED || k == CG_PROFILE_DROPPED || k == CG_PROFILE_RUNNING;
  const bool lock = k == CG_PROFILE_LOCK_GRANTED || k == CG_PROFILE_LOCK_SKIPPED || k == CG_PROFILE_LOCK_RUNNING;
  ms(KT_PF_RULES, PFEV_RULES, c->pfev[PFEV_WALK]);
  ms(KT_PF_WALK, PFEV_WALK, c->pfev[admission || lock ? PFEV_PREPARE : PFEV_TOTALS]);
  ms(KT_PF_TOTALS, PFEV_TOTALS, c->pfev[PFEV_TOTALS_END]);
  if (admission || lock) {  // the unit kernels sit between the walked runs and the totals
    ms(KT_UNIT_PREPARE, PFEV_PREPARE, c->pfev[PFEV_UNITS]);
    ms(admission ? KT_ADMIT_UNITS : KT_LOCK_UNITS, PFEV_UNITS, walk_end_event(c, running));
  }
  if (running) ms(KT_ROWS_PREFIX, PFEV_PREFIX, c->pfev[PFEV_TOTALS]);
  // the count and scan behind it, when the chain recorded their events
  if (c->phase_timing >= 2 && c->pf_R > 0) {
    (void)hipEventElapsedTime(&c->kt[KT_X_COUNT], c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->kt[KT_X_SCAN], c->ev[1], c->ev[2]);
  }
}

int profile_no_result() { return cg_fail(CG_EINVAL, "no profile result (the last profile call failed, or none was made)"); }

// an in-flight call's durations: ms [R] checked, -> whole seconds rounded up,
// clamped to the horizon (so INT64_MAX ms is valid and e - d cannot overflow)
int inflight_durations(const char* what, const cg_specs* s, const int64_t* dur_ms, int64_t horizon,
                       std::vector<int64_t>* dsec) {
  const size_t R = s->n;
  if (R > 0 && !dur_ms) return cg_fail(CG_EINVAL, std::string(what) + ": rule 0: null dur_ms");
  dsec->resize(R);
  for (size_t r = 0; r < R; r++) {
    if (dur_ms[r] < 0)
      return cg_fail(CG_EINVAL, std::string(what) + ": rule " + std::to_string(r) + ": negative duration");
    (*dsec)[r] = inflight_seconds(dur_ms[r], horizon);
  }
  return CG_OK;
}

// the node matrix of the rule matrix just enqueued, behind it on the stream
int profile_nodes_enqueue(cg_ctx* c, const RulesStore& in, int mode, int32_t B, bool cached, int64_t* nnz) {
  hipStream_t st = c->st;
  const int32_t N = in.n_nodes;
  int rc;
  // the rule->node join and its transpose: the per-node path's cache, keyed
  // by (rule set, exclude mode); rebuilt here on a miss (the cached segment
  // bounds go with the old transpose), its keys set once the stream drained
  if (!cached) {
    c->pn_cache_serial = 0;
    c->pn_K = 0;
    if ((rc = rule_nodes_locked(c, in, mode, nnz)) || (rc = transpose_locked(c, *nnz, N))) return rc;
  }
  (void)hipEventRecord(c->pfev[PFEV_NODES], st);
  const int64_t chunks_max = int64_t(N) + *nnz / kNodeChunk + 1;  // >= the chunk total
  if ((rc = c->pf_nodes.ensure(size_t(std::max<int64_t>(int64_t(N) * B, 1)))) ||
      (rc = c->pf_part.ensure(size_t(chunks_max * B))) || (rc = c->pf_chunk_cnt.ensure(size_t(std::max(N, 1)))) ||
      (rc = c->pf_chunk_off.ensure(size_t(N) + 1)) ||
      (rc = c->scan_tmp.ensure(std::max(c->scan_tmp.cap, scan_temp_bytes(std::max(N, 1))))))
    return rc;
  if (N > 0) {
    hipLaunchKernelGGL(k_profile_chunks, dim3(gridn(N, 256, 1 << 30)), dim3(256), 0, st, c->nt_off.p, N,
                       c->pf_chunk_cnt.p);
    launch_scan(c->pf_chunk_cnt.p, c->pf_chunk_off.p, N, c->scan_tmp.p, st);
    hipLaunchKernelGGL(k_profile_nodes, dim3(unsigned(chunks_max), (B + 63) / 64), dim3(256), 0, st, c->nt_off.p,
                       c->nt_rule.p, c->pf_chunk_off.p, N, c->pf_rules.p, B, c->pf_nodes.p, c->pf_part.p);
    hipLaunchKernelGGL(k_profile_nodes_reduce, dim3(gridn(int64_t(N) * B, 256, 1 << 30)), dim3(256), 0, st,
                       c->pf_chunk_off.p, N, B, c->pf_part.p, c->pf_nodes.p);
  }
  (void)hipEventRecord(c->pfev[PFEV_NODES_END], st);
  HIPCHK(hipGetLastError());
  return CG_OK;
}

// A profile call of any kind, arguments checked; rules null: the flat flavour,
// no node matrix.  Copies on the stream read the entry point's locals (durations,
// units, flags): a call that fails before its synchronise drains the stream.
int profile_call(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t B,
                 const ProfileCall& pc, const cg_rules* rules, int mode) {
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  const RulesStore* in = rules ? &rules->st : nullptr;
  int64_t nnz = c->pn_nnz;
  int rc = profile_rules_enqueue(c, s, z, t0, width, B, pc);
  const bool cached = in && in->serial != 0 && in->serial == c->pn_cache_serial && mode == c->pn_cache_mode;
  if (!rc && in) rc = profile_nodes_enqueue(c, *in, mode, B, cached, &nnz);
  if (!rc) rc = cg_hip_check(hipStreamSynchronize(c->st), "hipStreamSynchronize(c->st)");
  if (rc) {
    (void)hipStreamSynchronize(c->st);
    return rc;
  }
  profile_rule_times(c);
  if (in) {
    if (!cached) {
      c->pn_nnz = nnz;
      c->pn_cache_serial = in->serial;
      c->pn_cache_mode = mode;
      (void)hipEventElapsedTime(&c->kt[KT_PF_JOIN], c->pfev[PFEV_TOTALS_END], c->pfev[PFEV_NODES]);
    }
    (void)hipEventElapsedTime(&c->kt[KT_PF_NODES], c->pfev[PFEV_NODES], c->pfev[PFEV_NODES_END]);
    c->pf_N = in->n_nodes;
    c->pf_nnz = nnz;
    c->pf_nt_gen = c->nt_gen;  // the transpose the node matrix was summed from
    c->pf_has_nodes = true;
  }
  c->pf_valid = true;
  return CG_OK;
}

// what the eight entry points check first: the bucket arguments, then a
// per-node flavour's node arguments; the kind's own (durations / units) follow
int profile_prelude(const char* fn, const cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t width,
                    int32_t n_buckets, bool per_node = false, const cg_rules* rules = nullptr, int mode = 0) {
  if (int rc = profile_check_args(fn, c, s, z, width, n_buckets)) return rc;
  if (!per_node) return CG_OK;
  if (!rules) return cg_fail(CG_EINVAL, std::string(fn) + ": null");
  if (mode < 0 || mode > 2) return cg_fail(CG_EINVAL, "bad exclude mode");
  if (int64_t(s->n) != rules->st.n_rules) return cg_fail(CG_EINVAL, "specs count != rules n_rules");
  return CG_OK;
}

}  // namespace

int profile_node_peaks_enqueue(cg_ctx* c) {
  hipLaunchKernelGGL(k_node_peaks, dim3(gridn(c->pf_N, 4, 1 << 30)), dim3(256), 0, c->st, c->pf_nodes.p, c->pf_N,
                     c->pf_B, c->pf_peak.p, c->pf_peak_bucket.p);
  HIPCHK(hipGetLastError());
  return CG_OK;
}

extern "C" {

int cg_profile_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets) {
  if (int rc = profile_prelude("cg_profile_device", c, s, z, width, n_buckets)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall(), nullptr, 0);
}

int cg_profile_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                               int32_t n_buckets, const cg_rules* rules, int mode) {
  if (int rc = profile_prelude("cg_profile_per_node_device", c, s, z, width, n_buckets, true, rules, mode)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall(), rules, mode);
}

int cg_inflight_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets,
                       const int64_t* dur_ms) {
  const char* fn = "cg_inflight_device";
  std::vector<int64_t> dsec;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets)) return rc;
  if (int rc = inflight_durations(fn, s, dur_ms, int64_t(n_buckets) * width, &dsec)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::inflight(&dsec), nullptr, 0);
}

int cg_inflight_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                                int32_t n_buckets, const int64_t* dur_ms, const cg_rules* rules, int mode) {
  const char* fn = "cg_inflight_per_node_device";
  std::vector<int64_t> dsec;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets, true, rules, mode)) return rc;
  if (int rc = inflight_durations(fn, s, dur_ms, int64_t(n_buckets) * width, &dsec)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::inflight(&dsec), rules, mode);
}

int cg_admit_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets,
                    const int64_t* dur_ms, const int64_t* parallels, const int32_t* unit, int what) {
  const char* fn = "cg_admit_device";
  AdmitCall adm;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets)) return rc;
  if (int rc = admit_units(fn, s, dur_ms, parallels, unit, what, int64_t(n_buckets) * width, &adm)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::admission(&adm), nullptr, 0);
}

int cg_admit_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                             int32_t n_buckets, const int64_t* dur_ms, const int64_t* parallels,
                             const int32_t* unit, int what, const cg_rules* rules, int mode) {
  const char* fn = "cg_admit_per_node_device";
  AdmitCall adm;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets, true, rules, mode)) return rc;
  if (int rc = admit_units(fn, s, dur_ms, parallels, unit, what, int64_t(n_buckets) * width, &adm)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::admission(&adm), rules, mode);
}

int cg_lock_profile_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                           int32_t n_buckets, const int32_t* kind, const int64_t* avg_time_ms, const int32_t* unit,
                           const uint8_t* contends, int64_t lock_ttl, int what) {
  const char* fn = "cg_lock_profile_device";
  LockCall lk;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets)) return rc;
  if (int rc = lock_units(fn, s, kind, avg_time_ms, unit, contends, lock_ttl, what, int64_t(n_buckets) * width, &lk))
    return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::lock(&lk), nullptr, 0);
}

int cg_lock_profile_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                                    int32_t n_buckets, const int32_t* kind, const int64_t* avg_time_ms,
                                    const int32_t* unit, const uint8_t* contends, int64_t lock_ttl, int what,
                                    const cg_rules* rules, int mode) {
  const char* fn = "cg_lock_profile_per_node_device";
  LockCall lk;
  if (int rc = profile_prelude(fn, c, s, z, width, n_buckets, true, rules, mode)) return rc;
  if (int rc = lock_units(fn, s, kind, avg_time_ms, unit, contends, lock_ttl, what, int64_t(n_buckets) * width, &lk))
    return rc;
  return profile_call(c, s, z, t0, width, n_buckets, ProfileCall::lock(&lk), rules, mode);
}

int cg_profile_kind(cg_ctx* c, int* kind) {
  if (!c || !kind) return cg_fail(CG_EINVAL, "cg_profile_kind: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  *kind = c->pf_kind;
  return CG_OK;
}

int cg_profile_node_peaks(cg_ctx* c, int32_t first_node, int32_t count, int64_t* peak, int32_t* bucket) {
  if (!c || (count > 0 && (!peak || !bucket))) return cg_fail(CG_EINVAL, "cg_profile_node_peaks: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  if (!c->pf_has_nodes) return cg_fail(CG_EINVAL, "the last profile has no node matrix (no per-node call)");
  if (first_node < 0 || count < 0 || int64_t(first_node) + count > c->pf_N)
    return cg_fail(CG_EINVAL, "node range outside the last profile");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  const int32_t N = c->pf_N;
  if (!c->pf_peaks_valid && N > 0) {
    int rc;
    if ((rc = c->pf_peak.ensure(size_t(N))) || (rc = c->pf_peak_bucket.ensure(size_t(N)))) return rc;
    if ((rc = profile_node_peaks_enqueue(c))) return rc;
    HIPCHK(hipStreamSynchronize(c->st));
    c->pf_peaks_valid = true;
  }
  if (count) {
    HIPCHK(hipMemcpy(peak, c->pf_peak.p + first_node, size_t(count) * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(bucket, c->pf_peak_bucket.p + first_node, size_t(count) * 4, hipMemcpyDeviceToHost));
  }
  return CG_OK;
}

int cg_profile_result_device(cg_ctx* c, const int32_t** d_rule_counts, const int64_t** d_bucket_totals,
                             const int64_t** d_node_counts, int64_t* n_rules, int32_t* n_nodes, int32_t* n_buckets) {
  if (!c) return cg_fail(CG_EINVAL, "cg_profile_result_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  if (d_rule_counts) *d_rule_counts = c->pf_rules.p;
  if (d_bucket_totals) *d_bucket_totals = c->pf_totals.p;
  if (d_node_counts) *d_node_counts = c->pf_has_nodes ? c->pf_nodes.p : nullptr;
  if (n_rules) *n_rules = c->pf_R;
  if (n_nodes) *n_nodes = c->pf_has_nodes ? c->pf_N : 0;
  if (n_buckets) *n_buckets = c->pf_B;
  return CG_OK;
}

int cg_profile_copy_rules(cg_ctx* c, int64_t first_rule, int64_t count, int32_t* out) {
  if (!c || (count > 0 && !out)) return cg_fail(CG_EINVAL, "cg_profile_copy_rules: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  if (first_rule < 0 || count < 0 || first_rule + count > c->pf_R)
    return cg_fail(CG_EINVAL, "rule range outside the last profile");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (count)
    HIPCHK(hipMemcpy(out, c->pf_rules.p + first_rule * c->pf_B, size_t(count) * c->pf_B * 4, hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_profile_copy_totals(cg_ctx* c, int64_t* out) {
  if (!c || !out) return cg_fail(CG_EINVAL, "cg_profile_copy_totals: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(out, c->pf_totals.p, size_t(c->pf_B) * 8, hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_profile_copy_nodes(cg_ctx* c, int32_t first_node, int32_t count, int64_t* out) {
  if (!c || (count > 0 && !out)) return cg_fail(CG_EINVAL, "cg_profile_copy_nodes: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return profile_no_result();
  if (!c->pf_has_nodes) return cg_fail(CG_EINVAL, "the last profile has no node matrix (cg_profile_device)");
  if (first_node < 0 || count < 0 || int64_t(first_node) + count > c->pf_N)
    return cg_fail(CG_EINVAL, "node range outside the last profile");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (count)
    HIPCHK(hipMemcpy(out, c->pf_nodes.p + int64_t(first_node) * c->pf_B, size_t(count) * c->pf_B * 8,
                     hipMemcpyDeviceToHost));
  return CG_OK;
}

}  // extern "C"
