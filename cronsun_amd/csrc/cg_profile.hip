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
// Admission profile (cg_admit_*): the fires Job.limit() would admit, or those it
// would drop.  The start profile's first two kernels fill the rule matrix, then
//   k_admit_prepare   one lane per cell: zeroes the rows the kind rewrites
//                     (ADMITTED: of units that can drop; DROPPED: of the others)
//   k_admit_units     one lane per unit that can drop: walks the unit's
//                     admitted fires (cg_admit.h, admit_walk_unit) and adds
//                     (ADMITTED) or subtracts (DROPPED) 1 in the rule's own row
// and totals, node matrix and accessors are shared.
//
// Lock profile (cg_lock_profile_*): the fires the KindAlone / KindInterval
// lock of Cmd.Run would grant, or those it would skip.  The admission chain
// with the unit walk replaced:
//   k_admit_prepare   flag = contending rule of a lock unit (GRANTED: those
//                     rows restart from zero; SKIPPED: all other rows are zero)
//   k_lock_units      one lane per lock unit with a contending rule: walks the
//                     unit's granted fires (cg_lock.h, lock_walk_unit) and adds
//                     (GRANTED) or subtracts (SKIPPED) 1 in the rule's own row
//
// Running profile (CG_PROFILE_RUNNING / CG_PROFILE_LOCK_RUNNING): commands in
// flight counting only the fires that start.  The in-flight chain's first two
// kernels fill the rule matrix with every rule's d, then
//   k_admit_prepare   zeroes the flagged rows
//   k_admit_units / k_lock_units  in difference mode: +1 at the bucket a started
//                     fire comes into flight, -1 where it has ended
//                     (cg_profile.h, running_emit_diff)
//   k_rows_prefix     in-place inclusive prefix sum along each flagged row
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_admit.h"
#include "cg_lock.h"
#include "cg_profile.h"
#include "cg_stage.h"
#include "cg_units.h"

using namespace cg;

namespace {

constexpr int kMaxBuckets = 4096;
// rules of a node's list (k_profile_nodes: kNodeChunk, cg_api_internal.h) /
// rows of the rule matrix (k_profile_totals) summed by one block per bucket tile
constexpr int kTotalChunk = 4096;
static_assert(kAdmitMaxParallels == CG_ADMIT_MAX_PARALLELS, "cg_admit.h and the public header disagree");
static_assert(sizeof(AdmitUnit) == 24, "AdmitUnit is uploaded as 24-byte records");
static_assert(sizeof(LockUnit) == 32, "LockUnit is uploaded as 32-byte records");
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

// One lane per unit that can drop (units [U], compacted by the host so waves
// are dense); a block is one wave.  The lane walks the unit's admitted fires
// and adds `step` (+1 ADMITTED, -1 DROPPED: start - admitted) to the cell of
// the firing rule's row -- rows belong to one unit, so plain read-modify-write.
// With diff != 0 (RUNNING) it writes the fire's difference over its run time
// u.d instead (cg_profile.h, running_emit_diff) and step is not read.
// The ring of the last P admitted starts and the walked runs' remembered
// positions (cg_admit.h) live in LDS behind the staged plan, [slot][lane]: a
// lane's slots are 512 B (256 B) apart, conflict-free at any head.
constexpr int kAdmitBlock = 64;
__global__ __launch_bounds__(kAdmitBlock) void k_admit_units(const DSpec* __restrict__ specs, PlanArgs p,
                                                              const int64_t* __restrict__ run_anchor,
                                                              const int32_t* __restrict__ run_count,
                                                              const uint32_t* __restrict__ run_dmask,
                                                              const AdmitUnit* __restrict__ units, int64_t U,
                                                              size_t ring_off, int64_t w, int32_t B, int32_t step,
                                                              int32_t diff, int32_t* __restrict__ out) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  // [ring 16][walk t 8] i64, then [rel 8][s 8][q 8] i32, each [slot][lane]
  int64_t* ring = reinterpret_cast<int64_t*>(lds + ring_off) + threadIdx.x;
  int32_t* w32 = reinterpret_cast<int32_t*>(ring - threadIdx.x + (kAdmitMaxParallels + kAdmitWalkSlots) * kAdmitBlock) +
                 threadIdx.x;
  const AdmitWalkCache wc{ring + kAdmitMaxParallels * kAdmitBlock, w32, w32 + kAdmitWalkSlots * kAdmitBlock,
                          w32 + 2 * kAdmitWalkSlots * kAdmitBlock, kAdmitBlock};
  const int64_t i = blockIdx.x * int64_t(kAdmitBlock) + threadIdx.x;
  if (i >= U) return;
  const AdmitUnit u = units[i];
  const int64_t t0 = p.t0;
  admit_walk_unit(specs, v.z, v.segs, p.G, run_anchor, run_count, run_dmask, t0, p.t1, u, ring, kAdmitBlock, wc,
                  [&](int64_t r, int64_t t) {
                    if (diff) {  // RUNNING: the fire's difference, summed by k_rows_prefix
                      running_emit_diff(out + r * B, B, t, u.d, t0, w);
                      return;
                    }
                    const int64_t b = (t - t0 - 1) / w;
                    if (t > t0 && b < B) out[r * B + b] += step;
                  });
}

// ----------------------------------------------------------- lock profile --
// One lane per lock unit with a contending rule (units [U], compacted by the
// host so waves are dense); a block is one wave.  The lane walks the unit's
// granted fires and adds `step` (+1 GRANTED, -1 SKIPPED: start - granted) to
// the cell of the firing rule's row -- a row belongs to one unit, so plain
// read-modify-write.  With diff != 0 (LOCK_RUNNING) it writes the fire's
// difference over u.d instead, as k_admit_units does.  contends [R]: the prepare pass's flags, inside a lock
// unit "this rule reaches the lock".  The walked runs' remembered positions
// (cg_admit.h) live in LDS behind the staged plan, [slot][lane]; there is no
// ring.  A rule whose Next never returns lowers *stuck to its index.
constexpr int kLockBlock = 64;
__global__ __launch_bounds__(kLockBlock) void k_lock_units(const DSpec* __restrict__ specs, PlanArgs p,
                                                            const int64_t* __restrict__ run_anchor,
                                                            const int32_t* __restrict__ run_count,
                                                            const uint32_t* __restrict__ run_dmask,
                                                            const LockUnit* __restrict__ units, int64_t U,
                                                            const uint8_t* __restrict__ contends, size_t cache_off,
                                                            int64_t lock_ttl, int64_t w, int32_t B, int32_t step,
                                                            int32_t diff, int32_t* __restrict__ out,
                                                            unsigned long long* __restrict__ stuck) {
  extern __shared__ __align__(16) char lds[];
  PlanView v = stage_plan(p, lds);
  // [walk t 8] i64, then [rel 8][s 8][q 8] i32, each [slot][lane]
  int64_t* wt = reinterpret_cast<int64_t*>(lds + cache_off) + threadIdx.x;
  int32_t* w32 = reinterpret_cast<int32_t*>(lds + cache_off + size_t(kAdmitWalkSlots) * kLockBlock * 8) + threadIdx.x;
  const AdmitWalkCache wc{wt, w32, w32 + kAdmitWalkSlots * kLockBlock, w32 + 2 * kAdmitWalkSlots * kLockBlock,
                          kLockBlock};
  const int64_t i = blockIdx.x * int64_t(kLockBlock) + threadIdx.x;
  if (i >= U) return;
  const LockUnit u = units[i];
  const int64_t t0 = p.t0;
  const int64_t bad = lock_walk_unit(specs, v.z, v.segs, p.G, run_anchor, run_count, run_dmask, t0, p.t1, u, lock_ttl,
                                     contends, wc, [&](int64_t r, int64_t t) {
                                       if (diff) {  // LOCK_RUNNING: the command runs u.d whatever its lease does
                                         running_emit_diff(out + r * B, B, t, u.d, t0, w);
                                         return;
                                       }
                                       const int64_t b = (t - t0 - 1) / w;
                                       if (t > t0 && b < B) out[r * B + b] += step;
                                     });
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

int ensure_events(cg_ctx* c) {
  for (hipEvent_t& e : c->pfev)
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  return CG_OK;
}

// count chain + rule matrix + totals, enqueued on the ctx stream (the caller
// drains it); c->mu held.  pfev[0..3] bracket the three kernels (pfev[3]:
// the end of the totals, where a per-node call's join starts).  dsec: null for
// the start profile, else the in-flight profile's durations (host, [R], whole
// seconds clamped to B * w), uploaded here and read by this call's kernels only;
// it comes together with adm or lk in a RUNNING call, whose base rows are the
// in-flight profile's and whose unit walk writes differences that k_rows_prefix
// sums (pfev[8]: the end of that walk; pfev[2] then follows the prefix).
// adm / lk: an admission or a lock call's checked arguments (cg_units.h).
int profile_rules_enqueue(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t w, int32_t B,
                          const std::vector<int64_t>* dsec, const AdmitCall* adm = nullptr,
                          const LockCall* lk = nullptr) {
  c->pf_valid = false;
  c->pf_has_nodes = false;
  c->pf_peaks_valid = false;
  c->tr_valid = false;  // a top-rules result does not outlive its profile
  int rc;
  bool empty = true;
  if ((rc = sync_count_scan(c, s, z, t0, t0 + int64_t(B) * w, &empty, 0, lk != nullptr))) return rc;
  if ((rc = ensure_events(c))) return rc;
  const int64_t R = int64_t(s->n);
  if ((rc = c->pf_rules.ensure(size_t(std::max<int64_t>(R * B, 1)))) || (rc = c->pf_totals.ensure(size_t(B))))
    return rc;
  hipStream_t st = c->st;
  HIPCHK(hipMemsetAsync(c->pf_totals.p, 0, size_t(B) * 8, st));
  for (int i = 14; i < 23; i++) c->kt[i] = 0.f;
  const bool running = (adm && adm->running()) || (lk && lk->running());
  hipEvent_t walk_end = c->pfev[running ? 8 : 2];
  for (int i : {0, 1, 6, 7}) (void)hipEventRecord(c->pfev[i], st);
  if (running) (void)hipEventRecord(walk_end, st);
  for (int i : {2, 3}) (void)hipEventRecord(c->pfev[i], st);
  if (!empty) {
    RunSet& rs = c->rs;
    // a rule whose reference loop never ends: refuse before any cell is computed
    HIPCHK(hipStreamSynchronize(st));
    const unsigned long long stuck = static_cast<unsigned long long>(rs.res_host[1]);
    if (stuck != ~0ULL) return cg_fail(CG_ERANGE, stuck_msg(stuck));
    const size_t lds = plan_lds_bytes(rs.pa);
    const size_t cache_off = align_up(lds, 16), lock_lds = cache_off + size_t(kLockBlock) * kLockLaneBytes;
    if (lk && !lk->units.empty() && lock_lds > 64 * 1024)
      return cg_fail(CG_ERANGE, "cg_lock_profile: the plan of this horizon leaves no LDS for the walked runs' positions");
    if (dsec) {
      // (*dsec outlives the stream synchronise that ends the call)
      if ((rc = c->pf_dur.ensure(size_t(R)))) return rc;
      HIPCHK(hipMemcpyAsync(c->pf_dur.p, dsec->data(), size_t(R) * 8, hipMemcpyHostToDevice, st));
    }
    (void)hipEventRecord(c->pfev[0], st);
    if (dsec)
      hipLaunchKernelGGL(k_inflight_rules, dim3(gridn(R * B, 256, 4096)), dim3(256), lds, st, s->d, R, rs.pa,
                         rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, c->pf_dur.p, w, B, c->pf_rules.p);
    else
      hipLaunchKernelGGL(k_profile_rules, dim3(gridn(R * B, 256, 4096)), dim3(256), lds, st, s->d, R, rs.pa,
                         rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, w, B, c->pf_rules.p);
    (void)hipEventRecord(c->pfev[1], st);
    if (rs.has_walk()) {
      if (dsec)
        hipLaunchKernelGGL(k_inflight_walk, dim3(gridn(R, 256, 256 * 16)), dim3(256), lds, st, s->d, R, rs.pa,
                           rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, c->pf_dur.p, w, B, c->pf_rules.p);
      else
        hipLaunchKernelGGL(k_profile_walk, dim3(gridn(R, 256, 256 * 16)), dim3(256), lds, st, s->d, R, rs.pa,
                           rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, w, B, c->pf_rules.p);
    }
    if (adm) {
      // the start rows are in place: rewrite them on the same stream
      const int64_t U = int64_t(adm->units.size());
      const size_t ring_off = align_up(lds, 16), admit_lds = ring_off + size_t(kAdmitBlock) * kAdmitLaneBytes;
      if (U > 0 && admit_lds > 64 * 1024) return cg_fail(CG_ERANGE, "cg_admit: the plan of this horizon leaves no LDS for the admission ring");
      if ((rc = c->pf_admit_flag.ensure(size_t(R))) || (rc = c->pf_admit_units.ensure(size_t(std::max<int64_t>(U, 1)) * sizeof(AdmitUnit))))
        return rc;
      HIPCHK(hipMemcpyAsync(c->pf_admit_flag.p, adm->flag.data(), size_t(R), hipMemcpyHostToDevice, st));
      if (U > 0)
        HIPCHK(hipMemcpyAsync(c->pf_admit_units.p, adm->units.data(), size_t(U) * sizeof(AdmitUnit), hipMemcpyHostToDevice, st));
      (void)hipEventRecord(c->pfev[6], st);
      hipLaunchKernelGGL(k_admit_prepare, dim3(gridn(R * B, 256, 4096)), dim3(256), 0, st, c->pf_admit_flag.p, R, B,
                         adm->what != CG_PROFILE_DROPPED ? 1 : 0, c->pf_rules.p);
      (void)hipEventRecord(c->pfev[7], st);
      if (U > 0)
        hipLaunchKernelGGL(k_admit_units, dim3(unsigned((U + kAdmitBlock - 1) / kAdmitBlock)), dim3(kAdmitBlock), admit_lds,
                           st, s->d, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p,
                           reinterpret_cast<const AdmitUnit*>(c->pf_admit_units.p), U, ring_off, w, B,
                           adm->what == CG_PROFILE_DROPPED ? -1 : 1, running ? 1 : 0, c->pf_rules.p);
    }
    if (lk) {
      const int64_t U = int64_t(lk->units.size());
      if ((rc = c->pf_admit_flag.ensure(size_t(R))) ||
          (rc = c->pf_admit_units.ensure(size_t(std::max<int64_t>(U, 1)) * sizeof(LockUnit))) ||
          (rc = c->pf_lock_stuck.ensure(1)))
        return rc;
      HIPCHK(hipMemcpyAsync(c->pf_admit_flag.p, lk->flag.data(), size_t(R), hipMemcpyHostToDevice, st));
      if (U > 0)
        HIPCHK(hipMemcpyAsync(c->pf_admit_units.p, lk->units.data(), size_t(U) * sizeof(LockUnit), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(c->pf_lock_stuck.p, 0xFF, sizeof(unsigned long long), st));
      (void)hipEventRecord(c->pfev[6], st);
      hipLaunchKernelGGL(k_admit_prepare, dim3(gridn(R * B, 256, 4096)), dim3(256), 0, st, c->pf_admit_flag.p, R, B,
                         lk->what != CG_PROFILE_LOCK_SKIPPED ? 1 : 0, c->pf_rules.p);
      (void)hipEventRecord(c->pfev[7], st);
      if (U > 0)
        hipLaunchKernelGGL(k_lock_units, dim3(unsigned((U + kLockBlock - 1) / kLockBlock)), dim3(kLockBlock), lock_lds, st,
                           s->d, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p,
                           reinterpret_cast<const LockUnit*>(c->pf_admit_units.p), U, c->pf_admit_flag.p, cache_off,
                           lk->lock_ttl, w, B, lk->what == CG_PROFILE_LOCK_SKIPPED ? -1 : 1, running ? 1 : 0,
                           c->pf_rules.p, c->pf_lock_stuck.p);
      (void)hipEventRecord(walk_end, st);
      HIPCHK(hipGetLastError());
      // a granted fire whose Next never returns: the reference hangs in
      // lockTtl there, and the unit's rows are unfinished -- no profile
      unsigned long long lstuck = ~0ULL;
      HIPCHK(hipMemcpyAsync(&lstuck, c->pf_lock_stuck.p, sizeof lstuck, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (lstuck != ~0ULL)
        return cg_fail(CG_ERANGE, "cg_lock_profile: rule " + std::to_string(lstuck) +
                                      ": Next never returns from a fire of this horizon that finds the lock free "
                                      "(the reference's lockTtl does not return there)");
    } else {
      (void)hipEventRecord(walk_end, st);
    }
    if (running) {
      // the flagged rows hold differences: sum them along the buckets (rows of
      // a call without a unit to walk are all unflagged)
      const int rows_per_block = B >= 64 ? 4 : 4 * (64 / B);
      if ((adm ? adm->units.size() : lk->units.size()) > 0)
        hipLaunchKernelGGL(k_rows_prefix, dim3(gridn(R, rows_per_block, 4096)), dim3(256), 0, st, c->pf_admit_flag.p, R,
                           B, c->pf_rules.p);
      (void)hipEventRecord(c->pfev[2], st);
    }
    hipLaunchKernelGGL(k_profile_totals, dim3(gridn(R, kTotalChunk, 1 << 30), (B + 63) / 64), dim3(256), 0, st,
                       c->pf_rules.p, R, B, reinterpret_cast<unsigned long long*>(c->pf_totals.p));
    (void)hipEventRecord(c->pfev[3], st);
    HIPCHK(hipGetLastError());
  }
  c->pf_R = R;
  c->pf_B = B;
  c->pf_N = 0;
  c->pf_kind = lk ? lk->what : adm ? adm->what : dsec ? CG_PROFILE_INFLIGHT : CG_PROFILE_STARTS;
  return CG_OK;
}

void profile_rule_times(cg_ctx* c) {
  for (int i = 0; i < 3; i++) (void)hipEventElapsedTime(&c->kt[14 + i], c->pfev[i], c->pfev[i + 1]);
  const bool running = c->pf_kind == CG_PROFILE_RUNNING || c->pf_kind == CG_PROFILE_LOCK_RUNNING;
  hipEvent_t walk_end = c->pfev[running ? 8 : 2];
  if (c->pf_kind == CG_PROFILE_ADMITTED || c->pf_kind == CG_PROFILE_DROPPED || c->pf_kind == CG_PROFILE_RUNNING) {
    // the admission kernels sit between the walked runs and the totals
    (void)hipEventElapsedTime(&c->kt[15], c->pfev[1], c->pfev[6]);
    (void)hipEventElapsedTime(&c->kt[19], c->pfev[6], c->pfev[7]);
    (void)hipEventElapsedTime(&c->kt[20], c->pfev[7], walk_end);
  }
  if (c->pf_kind == CG_PROFILE_LOCK_GRANTED || c->pf_kind == CG_PROFILE_LOCK_SKIPPED ||
      c->pf_kind == CG_PROFILE_LOCK_RUNNING) {
    (void)hipEventElapsedTime(&c->kt[15], c->pfev[1], c->pfev[6]);
    (void)hipEventElapsedTime(&c->kt[19], c->pfev[6], c->pfev[7]);
    (void)hipEventElapsedTime(&c->kt[21], c->pfev[7], walk_end);
  }
  if (running) (void)hipEventElapsedTime(&c->kt[22], c->pfev[8], c->pfev[2]);  // k_rows_prefix
  // the count and scan behind it, when the chain recorded their events ([0], [1])
  if (c->phase_timing >= 2 && c->pf_R > 0) {
    (void)hipEventElapsedTime(&c->kt[0], c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->kt[1], c->ev[1], c->ev[2]);
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

// the rule-matrix call of either kind (dsec null: starts); arguments checked
int profile_call(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets,
                 const std::vector<int64_t>* dsec, const AdmitCall* adm = nullptr, const LockCall* lk = nullptr) {
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  int rc = profile_rules_enqueue(c, s, z, t0, width, n_buckets, dsec, adm, lk);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->st));
  profile_rule_times(c);
  c->pf_valid = true;
  return CG_OK;
}

int profile_check_node_args(const char* what, const cg_specs* s, const cg_rules* rules, int mode) {
  if (!rules) return cg_fail(CG_EINVAL, std::string(what) + ": null");
  if (mode < 0 || mode > 2) return cg_fail(CG_EINVAL, "bad exclude mode");
  if (int64_t(s->n) != rules->st.n_rules) return cg_fail(CG_EINVAL, "specs count != rules n_rules");
  return CG_OK;
}

// the per-node call of either kind; arguments checked
int profile_per_node_call(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                          int32_t n_buckets, const cg_rules* rules, int mode, const std::vector<int64_t>* dsec,
                          const AdmitCall* adm = nullptr, const LockCall* lk = nullptr) {
  const RulesStore& in = rules->st;
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  const int32_t B = n_buckets, N = in.n_nodes;
  int rc = profile_rules_enqueue(c, s, z, t0, width, B, dsec, adm, lk);
  if (rc) return rc;
  hipStream_t st = c->st;
  // the rule->node join and its transpose: the per-node path's cache, keyed
  // by (rule set, exclude mode); rebuilt here on a miss (the cached segment
  // bounds go with the old transpose), its keys set once the stream drained
  const bool cached = in.serial != 0 && in.serial == c->pn_cache_serial && mode == c->pn_cache_mode;
  int64_t nnz = c->pn_nnz;
  if (!cached) {
    c->pn_cache_serial = 0;
    c->pn_K = 0;
    if ((rc = rule_nodes_locked(c, in, mode, &nnz)) || (rc = transpose_locked(c, nnz, N))) return rc;
  }
  (void)hipEventRecord(c->pfev[4], st);
  const int64_t chunks_max = int64_t(N) + nnz / kNodeChunk + 1;  // >= the chunk total
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
  (void)hipEventRecord(c->pfev[5], st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  if (!cached) {
    c->pn_nnz = nnz;
    c->pn_cache_serial = in.serial;
    c->pn_cache_mode = mode;
  }
  profile_rule_times(c);
  if (!cached) (void)hipEventElapsedTime(&c->kt[17], c->pfev[3], c->pfev[4]);  // 0: the cached join was reused
  (void)hipEventElapsedTime(&c->kt[18], c->pfev[4], c->pfev[5]);
  c->pf_N = N;
  c->pf_nnz = nnz;
  c->pf_nt_gen = c->nt_gen;  // the transpose the node matrix was summed from
  c->pf_has_nodes = true;
  c->pf_valid = true;
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
  if (int rc = profile_check_args("cg_profile_device", c, s, z, width, n_buckets)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, nullptr);
}

int cg_profile_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                               int32_t n_buckets, const cg_rules* rules, int mode) {
  if (int rc = profile_check_args("cg_profile_per_node_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = profile_check_node_args("cg_profile_per_node_device", s, rules, mode)) return rc;
  return profile_per_node_call(c, s, z, t0, width, n_buckets, rules, mode, nullptr);
}

int cg_inflight_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets,
                       const int64_t* dur_ms) {
  std::vector<int64_t> dsec;
  if (int rc = profile_check_args("cg_inflight_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = inflight_durations("cg_inflight_device", s, dur_ms, int64_t(n_buckets) * width, &dsec)) return rc;
  return profile_call(c, s, z, t0, width, n_buckets, &dsec);
}

int cg_inflight_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                                int32_t n_buckets, const int64_t* dur_ms, const cg_rules* rules, int mode) {
  std::vector<int64_t> dsec;
  if (int rc = profile_check_args("cg_inflight_per_node_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = profile_check_node_args("cg_inflight_per_node_device", s, rules, mode)) return rc;
  if (int rc = inflight_durations("cg_inflight_per_node_device", s, dur_ms, int64_t(n_buckets) * width, &dsec))
    return rc;
  return profile_per_node_call(c, s, z, t0, width, n_buckets, rules, mode, &dsec);
}

int cg_admit_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width, int32_t n_buckets,
                    const int64_t* dur_ms, const int64_t* parallels, const int32_t* unit, int what) {
  AdmitCall adm;
  if (int rc = profile_check_args("cg_admit_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = admit_units("cg_admit_device", s, dur_ms, parallels, unit, what, int64_t(n_buckets) * width, &adm))
    return rc;
  return profile_call(c, s, z, t0, width, n_buckets, adm.durations(), &adm);
}

int cg_admit_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                             int32_t n_buckets, const int64_t* dur_ms, const int64_t* parallels,
                             const int32_t* unit, int what, const cg_rules* rules, int mode) {
  AdmitCall adm;
  if (int rc = profile_check_args("cg_admit_per_node_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = profile_check_node_args("cg_admit_per_node_device", s, rules, mode)) return rc;
  if (int rc = admit_units("cg_admit_per_node_device", s, dur_ms, parallels, unit, what, int64_t(n_buckets) * width,
                           &adm))
    return rc;
  return profile_per_node_call(c, s, z, t0, width, n_buckets, rules, mode, adm.durations(), &adm);
}

int cg_lock_profile_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                           int32_t n_buckets, const int32_t* kind, const int64_t* avg_time_ms, const int32_t* unit,
                           const uint8_t* contends, int64_t lock_ttl, int what) {
  LockCall lk;
  if (int rc = profile_check_args("cg_lock_profile_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = lock_units("cg_lock_profile_device", s, kind, avg_time_ms, unit, contends, lock_ttl, what,
                          int64_t(n_buckets) * width, &lk))
    return rc;
  return profile_call(c, s, z, t0, width, n_buckets, lk.durations(), nullptr, &lk);
}

int cg_lock_profile_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t width,
                                    int32_t n_buckets, const int32_t* kind, const int64_t* avg_time_ms,
                                    const int32_t* unit, const uint8_t* contends, int64_t lock_ttl, int what,
                                    const cg_rules* rules, int mode) {
  LockCall lk;
  if (int rc = profile_check_args("cg_lock_profile_per_node_device", c, s, z, width, n_buckets)) return rc;
  if (int rc = profile_check_node_args("cg_lock_profile_per_node_device", s, rules, mode)) return rc;
  if (int rc = lock_units("cg_lock_profile_per_node_device", s, kind, avg_time_ms, unit, contends, lock_ttl, what,
                          int64_t(n_buckets) * width, &lk))
    return rc;
  return profile_per_node_call(c, s, z, t0, width, n_buckets, rules, mode, lk.durations(), nullptr, &lk);
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
