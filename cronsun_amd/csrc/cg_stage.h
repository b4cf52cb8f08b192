// cg_stage.h -- what every plan-reading kernel starts with: the batch plan
// (zone table, segments, day table) staged into LDS, and a rule's packed spec
// loaded as two 16-byte words.  Shared by cg_kernels.hip and cg_profile.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "cg_kernels.h"
#include "cg_time.h"
#include "cg_zone.h"

namespace cg {

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- plan staging into LDS --------------------------------------------
struct PlanView {
  ZoneView z;
  const Segment* segs;
  const uint32_t* dtab;
};

__device__ inline PlanView stage_plan(const PlanArgs& p, char* lds) {
  int64_t* w = reinterpret_cast<int64_t*>(lds);
  int32_t* o = reinterpret_cast<int32_t*>(lds + align_up(size_t(p.zn) * 8, 16));
  Segment* s = reinterpret_cast<Segment*>(lds + align_up(size_t(p.zn) * 8, 16) +
                                          align_up(size_t(p.zn) * 4, 16));
  uint32_t* d = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s) +
                                            align_up(size_t(p.G) * sizeof(Segment), 16));
  for (int i = threadIdx.x; i < p.zn; i += blockDim.x) {
    w[i] = p.zwhen[i];
    o[i] = p.zoff[i];
  }
  const int64_t* sg = reinterpret_cast<const int64_t*>(p.segs);
  int64_t* sd = reinterpret_cast<int64_t*>(s);
  for (int i = threadIdx.x; i < p.G * int(sizeof(Segment) / 8); i += blockDim.x) sd[i] = sg[i];
  if (!p.dtab_global)
    for (int i = threadIdx.x; i < p.nd; i += blockDim.x) d[i] = p.dtab[i];
  __syncthreads();
  PlanView v;
  v.z.when = w;
  v.z.off = o;
  v.z.n = p.zn;
  v.segs = s;
  v.dtab = p.dtab_global ? p.dtab : d;
  return v;
}

__device__ __forceinline__ DSpec load_spec(const DSpec* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  DSpec s;
  s.sec = (uint64_t(a.y) << 32) | a.x;
  s.min = (uint64_t(a.w) << 32) | a.z;
  s.hour = b.x;
  s.dom = b.y;
  s.mondow = b.z;
  s.kind = b.w;
  return s;
}

}  // namespace cg
