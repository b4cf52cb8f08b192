// cg_unit_walk.h -- what the four unit-walk kernels share: k_admit_units,
// k_lock_units (cg_profile.hip), k_admit_verdicts, k_lock_verdicts
// (cg_verdict.hip).  A block is one wave of kUnitBlock lanes, one lane per
// compacted unit.  Behind the staged plan (cg_stage.h) the dynamic LDS holds a
// tail of per-lane state, every region [slot][lane], so a lane's slots are
// kUnitBlock elements apart (conflict-free at any index):
//   admission  ring [kAdmitMaxParallels][lane] i64 (the last P admitted
//              starts), then the walk cache;  lock: the walk cache alone
//   walk cache t [kAdmitWalkSlots][lane] i64, then rel, s, q [..][lane] i32
//              (cg_admit.h, AdmitWalkCache)
#pragma once
#include <hip/hip_runtime.h>

#include "cg_admit.h"
#include "cg_lock.h"
#include "cg_stage.h"

namespace cg {

constexpr int kUnitBlock = 64;

// byte offsets inside the walk cache, and of ring and walk cache inside the tail
constexpr size_t kRow64 = size_t(kUnitBlock) * 8, kRow32 = size_t(kUnitBlock) * 4;  // one slot of every lane
constexpr size_t kWalkTOff = 0, kWalkRelOff = kWalkTOff + kAdmitWalkSlots * kRow64;
constexpr size_t kWalkSOff = kWalkRelOff + kAdmitWalkSlots * kRow32, kWalkQOff = kWalkSOff + kAdmitWalkSlots * kRow32;
constexpr size_t kWalkBytes = kWalkQOff + kAdmitWalkSlots * kRow32;
constexpr size_t kAdmitRingOff = 0, kAdmitWalkOff = kAdmitRingOff + kAdmitMaxParallels * kRow64, kLockWalkOff = 0;
static_assert(kAdmitWalkOff + kWalkBytes == kUnitBlock * kAdmitLaneBytes, "admission tail != cg_admit.h's lane bytes");
static_assert(kLockWalkOff + kWalkBytes == kUnitBlock * kLockLaneBytes, "lock tail != cg_lock.h's lane bytes");
static_assert(kAdmitRingOff % 8 == 0 && (kAdmitWalkOff + kWalkTOff) % 8 == 0 && (kLockWalkOff + kWalkTOff) % 8 == 0,
              "the i64 regions start 8-byte aligned in a 16-byte aligned tail");

// where the tail starts behind a plan of plan_lds bytes, and the launch sizes
__host__ __device__ inline size_t unit_tail_off(size_t plan_lds) { return align_up(plan_lds, 16); }
__host__ __device__ inline size_t admit_lds_bytes(size_t plan_lds) {
  return unit_tail_off(plan_lds) + kAdmitWalkOff + kWalkBytes;
}
__host__ __device__ inline size_t lock_lds_bytes(size_t plan_lds) {
  return unit_tail_off(plan_lds) + kLockWalkOff + kWalkBytes;
}

// this lane's columns of the walk cache at `base`
__device__ __forceinline__ AdmitWalkCache walk_cache_view(char* base) {
  return AdmitWalkCache{reinterpret_cast<int64_t*>(base + kWalkTOff) + threadIdx.x,
                        reinterpret_cast<int32_t*>(base + kWalkRelOff) + threadIdx.x,
                        reinterpret_cast<int32_t*>(base + kWalkSOff) + threadIdx.x,
                        reinterpret_cast<int32_t*>(base + kWalkQOff) + threadIdx.x, kUnitBlock};
}
struct AdmitLdsView {
  int64_t* ring;  // slot i at ring[i * kUnitBlock]
  AdmitWalkCache wc;
};
__device__ __forceinline__ AdmitLdsView admit_lds_view(char* lds, size_t tail_off) {
  char* tail = lds + tail_off;
  return AdmitLdsView{reinterpret_cast<int64_t*>(tail + kAdmitRingOff) + threadIdx.x,
                      walk_cache_view(tail + kAdmitWalkOff)};
}
__device__ __forceinline__ AdmitWalkCache lock_lds_view(char* lds, size_t tail_off) {
  return walk_cache_view(lds + tail_off + kLockWalkOff);
}

// One lane of an admission walk kernel: stages the plan, takes unit
// blockIdx.x * kUnitBlock + threadIdx.x of units [U] and walks its admitted
// fires (cg_admit.h, admit_walk_unit): emit(plan view, unit, rule, time).
template <class Emit>
__device__ __forceinline__ void admit_unit_lane(const DSpec* __restrict__ specs, const PlanArgs& p,
                                                const int64_t* __restrict__ run_anchor,
                                                const int32_t* __restrict__ run_count,
                                                const uint32_t* __restrict__ run_dmask,
                                                const AdmitUnit* __restrict__ units, int64_t U, size_t tail_off,
                                                Emit&& emit) {
  extern __shared__ __align__(16) char lds[];
  const PlanView v = stage_plan(p, lds);
  const AdmitLdsView a = admit_lds_view(lds, tail_off);
  const int64_t i = blockIdx.x * int64_t(kUnitBlock) + threadIdx.x;
  if (i >= U) return;
  const AdmitUnit u = units[i];
  admit_walk_unit(specs, v.z, v.segs, p.G, run_anchor, run_count, run_dmask, p.t0, p.t1, u, a.ring, kUnitBlock, a.wc,
                  [&](int64_t r, int64_t t) { emit(v, u, r, t); });
}

// One lane of a lock walk kernel: the same over lock units and their granted
// fires (cg_lock.h, lock_walk_unit).  Returns -1, or the rule whose Next never
// returns (-1 in lanes past U).
template <class Emit>
__device__ __forceinline__ int64_t lock_unit_lane(const DSpec* __restrict__ specs, const PlanArgs& p,
                                                  const int64_t* __restrict__ run_anchor,
                                                  const int32_t* __restrict__ run_count,
                                                  const uint32_t* __restrict__ run_dmask,
                                                  const LockUnit* __restrict__ units, int64_t U, size_t tail_off,
                                                  const uint8_t* __restrict__ contends, int64_t lock_ttl,
                                                  Emit&& emit) {
  extern __shared__ __align__(16) char lds[];
  const PlanView v = stage_plan(p, lds);
  const AdmitWalkCache wc = lock_lds_view(lds, tail_off);
  const int64_t i = blockIdx.x * int64_t(kUnitBlock) + threadIdx.x;
  if (i >= U) return -1;
  const LockUnit u = units[i];
  return lock_walk_unit(specs, v.z, v.segs, p.G, run_anchor, run_count, run_dmask, p.t0, p.t1, u, lock_ttl, contends,
                        wc, [&](int64_t r, int64_t t) { emit(v, u, r, t); });
}

}  // namespace cg
