// cg_verdict.hip -- fire verdicts: one byte per fire of the rule-major
// expansion saying whether Job.limit() would drop it (bit 0, job.go:134-139,
// 165-187) and whether the KindAlone / KindInterval lock would skip it (bit 1,
// job.go:194-271), and the selection of the fires with given bits (DESIGN.md
// §5, "fire verdicts").  All on the ctx stream, behind the count -> scan ->
// writer chain of cg_expand_device:
//
//   k_verdict_init     every byte of verdict[0..E): the fire's rule flags (bit 0
//                      "unit can drop", bit 1 "contending rule of a lock unit");
//                      16 bytes per lane, a tile's rule range found by search
//                      over the rule offsets
//   k_admit_verdicts   k_admit_units' lane body (cg_unit_walk.h): one lane per
//                      unit that can drop walks the unit's admitted fires and
//                      clears bit 0 at fire_position (cg_verdict.h)
//   k_lock_verdicts    k_lock_units' lane body: one lane per lock unit with a
//                      contending rule walks the granted fires and clears bit 1
//   k_verdict_count    one wave per rule: fires with (v & mask) == value
//   launch_scan        their exclusive scan: sel_off [R+1]
//   k_verdict_select   one wave per rule: the matching fires' times, in order,
//                      compacted by ballot (stable, consecutive lanes store
//                      consecutive words)
//
// A rule belongs to one admission unit and to one lock unit, and the two walks
// run one after the other, so the byte read-modify-writes are lane-private.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_unit_walk.h"
#include "cg_units.h"
#include "cg_verdict.h"

using namespace cg;

namespace {

static_assert(kVerdictDropped == CG_VERDICT_DROPPED && kVerdictSkipped == CG_VERDICT_SKIPPED,
              "cg_verdict.h and the public header disagree");

// ---------------------------------------------------------------- init pass --
// largest r in [lo, hi] with off[r] <= e: the rule of fire index e when the
// range holds it (off[hi + 1] > e)
__device__ __forceinline__ int64_t rule_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A block takes tiles of kInitTile fires: two lanes search the rule range of
// the tile's first and last fire over all R + 1 offsets, every lane then the
// rule of its 16 fires inside that range (one rule for most tiles), and stores
// 16 bytes at once; the tail of the last tile goes byte by byte.
constexpr int kInitTile = 256 * 16;
__global__ __launch_bounds__(256) void k_verdict_init(const int64_t* __restrict__ offsets, int64_t R, int64_t E,
                                                       const uint8_t* __restrict__ flag,
                                                       uint8_t* __restrict__ verdict) {
  __shared__ int64_t range[2];
  const int64_t tiles = (E + kInitTile - 1) / kInitTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t e0 = tile * kInitTile, e1 = e0 + kInitTile < E ? e0 + kInitTile : E;
    if (threadIdx.x < 2) range[threadIdx.x] = rule_of(offsets, 0, R - 1, threadIdx.x ? e1 - 1 : e0);
    __syncthreads();
    const int64_t rlo = range[0], rhi = range[1];
    __syncthreads();
    const int64_t e = e0 + int64_t(threadIdx.x) * 16;
    if (e >= e1) continue;
    const int n = e1 - e < 16 ? int(e1 - e) : 16;
    int64_t r = rule_of(offsets, rlo, rhi, e);
    int64_t next = offsets[r + 1];
    uint32_t f = flag[r];
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      if (k < n) {
        if (e + k >= next) {  // past the rule's last fire: the next rule with one
          r = rule_of(offsets, r + 1, rhi, e + k);
          next = offsets[r + 1];
          f = flag[r];
        }
        w[k >> 2] |= f << (8 * (k & 3));
      }
    }
    if (n == 16) {
      *reinterpret_cast<uint4*>(verdict + e) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (k < n) verdict[e + k] = uint8_t(w[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// --------------------------------------------------------------- unit walks --
// what the clearing emit of both walks needs
struct VerdictOut {
  const int64_t* run_off;
  const int64_t* times;
  uint8_t* verdict;
  int64_t E;
  unsigned long long* err;  // [0]: lowered to a rule whose fire was not found where fire_position says
};

// clears `bit` of the byte of fire t of rule r; the position is checked against
// the fire list before the store (a self-check, not an expected path)
__device__ __forceinline__ void clear_verdict(const VerdictOut& o, const DSpec* __restrict__ specs,
                                              const Segment* segs, int G, const int64_t* run_anchor,
                                              const int32_t* run_count, const uint32_t* run_dmask, int64_t t1,
                                              int64_t r, int64_t t, uint8_t bit) {
  const int64_t j0 = r * G;
  const DSpec sp = specs[r];
  const int64_t pos =
      fire_position(sp, segs, G, run_anchor + j0, run_count + j0, run_dmask + j0, o.run_off + j0, o.times, t1, t);
  if (pos < 0 || pos >= o.E || o.times[pos] != t) {
    atomicMin(o.err, static_cast<unsigned long long>(r));
    return;
  }
  o.verdict[pos] &= uint8_t(~bit);
}

// the walks of k_admit_units / k_lock_units (cg_unit_walk.h) with the clearing
// emit; a rule whose Next never returns lowers err[1] to its index
__global__ __launch_bounds__(kUnitBlock) void k_admit_verdicts(const DSpec* __restrict__ specs, PlanArgs p,
                                                                const int64_t* __restrict__ run_anchor,
                                                                const int32_t* __restrict__ run_count,
                                                                const uint32_t* __restrict__ run_dmask,
                                                                const AdmitUnit* __restrict__ units, int64_t U,
                                                                size_t ring_off, VerdictOut o) {
  admit_unit_lane(specs, p, run_anchor, run_count, run_dmask, units, U, ring_off,
                  [&](const PlanView& v, const AdmitUnit&, int64_t r, int64_t t) {
                    clear_verdict(o, specs, v.segs, p.G, run_anchor, run_count, run_dmask, p.t1, r, t,
                                  kVerdictDropped);
                  });
}

__global__ __launch_bounds__(kUnitBlock) void k_lock_verdicts(const DSpec* __restrict__ specs, PlanArgs p,
                                                               const int64_t* __restrict__ run_anchor,
                                                               const int32_t* __restrict__ run_count,
                                                               const uint32_t* __restrict__ run_dmask,
                                                               const LockUnit* __restrict__ units, int64_t U,
                                                               const uint8_t* __restrict__ contends, size_t cache_off,
                                                               int64_t lock_ttl, VerdictOut o) {
  const int64_t bad = lock_unit_lane(specs, p, run_anchor, run_count, run_dmask, units, U, cache_off, contends,
                                     lock_ttl, [&](const PlanView& v, const LockUnit&, int64_t r, int64_t t) {
                                       clear_verdict(o, specs, v.segs, p.G, run_anchor, run_count, run_dmask, p.t1,
                                                     r, t, kVerdictSkipped);
                                     });
  if (bad >= 0) atomicMin(o.err + 1, static_cast<unsigned long long>(bad));
}

// ---------------------------------------------------------------- selection --
// one wave per rule, rules strided over the grid; a rule has fewer than 2^31
// fires (CG_MAX_HORIZON seconds), every index into the fires is 64-bit
__global__ __launch_bounds__(256) void k_verdict_count(const int64_t* __restrict__ offsets, int64_t R,
                                                        const uint8_t* __restrict__ verdict, uint32_t mask,
                                                        uint32_t value, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < R; r += int64_t(gridDim.x) * 4) {
    const int64_t b = offsets[r], e = offsets[r + 1];
    int32_t n = 0;
    for (int64_t i = b + lane; i < e; i += 64) n += (verdict[i] & mask) == value;
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    if (lane == 0) cnt[r] = n;
  }
}

__global__ __launch_bounds__(256) void k_verdict_select(const int64_t* __restrict__ offsets, int64_t R,
                                                         const uint8_t* __restrict__ verdict,
                                                         const int64_t* __restrict__ times, uint32_t mask,
                                                         uint32_t value, const int64_t* __restrict__ sel_off,
                                                         int64_t* __restrict__ sel_times) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ULL << lane) - 1;
  for (int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); r < R; r += int64_t(gridDim.x) * 4) {
    const int64_t b = offsets[r], e = offsets[r + 1];
    int64_t dst = sel_off[r];
    if (sel_off[r + 1] == dst) continue;  // a whole wave
    for (int64_t i0 = b; i0 < e; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool m = i < e && (verdict[i] & mask) == value;
      const unsigned long long bal = __ballot(m);
      if (m) sel_times[dst + __popcll(bal & below)] = times[i];
      dst += __popcll(bal);
    }
  }
}

// --------------------------------------------------------------------- host --
int no_verdicts() {
  return cg_fail(CG_EINVAL, "no fire verdicts (no verdict call has succeeded, or a later expansion call replaced "
                            "the result they belong to)");
}
bool verdicts_readable(const cg_ctx* c) { return c->vd_valid && c->vd_gen == c->res_gen; }
int no_selection() {
  return cg_fail(CG_EINVAL, "no verdict selection (no cg_verdicts_select_device since the last verdict call)");
}

int verdicts_locked(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1, const AdmitCall* adm,
                    const LockCall* lk, const std::vector<uint8_t>& flag, int64_t* n_events) {
  c->vd_valid = false;
  c->vd_sel_valid = false;
  for (float& x : c->vd_ms) x = 0.f;
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_events(c->vdev))) return rc;
  hipStream_t st = c->st;
  // the plain expansion; a lock call's count chain stages the lock table
  (void)hipEventRecord(c->vdev[VDEV_EXPAND], st);
  int64_t E = 0;
  if ((rc = expand_device_locked(c, s, z, t0, t1, &E, lk != nullptr))) return rc;
  for (int i = VDEV_INIT; i <= VDEV_WALKS_END; i++) (void)hipEventRecord(c->vdev[i], st);
  const int64_t R = int64_t(s->n);
  RunSet& rs = c->rs;
  if ((rc = c->vd_verdict.ensure(size_t(std::max<int64_t>(E, 1))))) return rc;
  if (E > 0) {
    const char* fn = "cg_expand_verdicts_device";
    const int64_t UA = adm ? int64_t(adm->units.size()) : 0, UL = lk ? int64_t(lk->units.size()) : 0;
    const size_t lds = plan_lds_bytes(rs.pa), tail_off = unit_tail_off(lds);
    if ((UA > 0 && (rc = admit_lds_check(fn, lds))) || (UL > 0 && (rc = lock_lds_check(fn, lds)))) return rc;
    if ((rc = unit_upload(c, R, UA > 0 ? adm : nullptr, UL > 0 ? lk : nullptr, flag.data(), true))) return rc;
    const VerdictOut o{rs.run_off.p, c->times.p, c->vd_verdict.p, E, c->uw_err.p};
    (void)hipEventRecord(c->vdev[VDEV_INIT], st);
    hipLaunchKernelGGL(k_verdict_init, dim3(gridn(E, kInitTile, 1 << 16)), dim3(256), 0, st, rs.offsets.p, R, E,
                       c->uw_flag[0].p, c->vd_verdict.p);
    (void)hipEventRecord(c->vdev[VDEV_ADMIT], st);
    if (UA > 0)
      hipLaunchKernelGGL(k_admit_verdicts, dim3(unsigned((UA + kUnitBlock - 1) / kUnitBlock)), dim3(kUnitBlock),
                         admit_lds_bytes(lds), st, s->d, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p,
                         uw_admit_units(c), UA, tail_off, o);
    (void)hipEventRecord(c->vdev[VDEV_LOCK], st);
    if (UL > 0)
      hipLaunchKernelGGL(k_lock_verdicts, dim3(unsigned((UL + kUnitBlock - 1) / kUnitBlock)), dim3(kUnitBlock),
                         lock_lds_bytes(lds), st, s->d, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p,
                         uw_lock_units(c), UL, c->uw_flag[1].p, tail_off, lk->lock_ttl, o);
    (void)hipEventRecord(c->vdev[VDEV_WALKS_END], st);
    HIPCHK(hipGetLastError());
    unsigned long long err[2];
    if ((rc = unit_errors(c, err))) return rc;
    if (err[1] != ~0ULL) return cg_fail(CG_ERANGE, lock_stuck_msg(fn, err[1]));
    if (err[0] != ~0ULL)
      return cg_fail(CG_EHIP, "verdict position mismatch: rule " + std::to_string(err[0]) +
                                  ": a fire of the unit walk is not where fire_position puts it in the result");
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int i = VDEV_EXPAND; i < VDEV_WALKS_END; i++)
    (void)hipEventElapsedTime(&c->vd_ms[i], c->vdev[i], c->vdev[i + 1]);
  c->vd_R = R;
  c->vd_E = E;
  c->vd_gen = c->res_gen;
  c->vd_valid = true;
  *n_events = E;
  return CG_OK;
}

}  // namespace

extern "C" {

int cg_expand_verdicts_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                              const cg_admit_args* admit, const cg_lock_args* lock, int64_t* n_events) {
  const char* fn = "cg_expand_verdicts_device";
  if (!c || !s || !z || !n_events) return cg_fail(CG_EINVAL, std::string(fn) + ": null");
  if (!admit && !lock) return cg_fail(CG_EINVAL, std::string(fn) + ": admit and lock are both NULL");
  const int64_t lim = int64_t(1) << 45;
  if (t0 < -lim || t0 > lim || t1 < -lim || t1 > lim || t1 - t0 > CG_MAX_HORIZON)
    return cg_fail(CG_ERANGE, "horizon must satisfy t1 - t0 <= CG_MAX_HORIZON (40 years)");
  if (t1 <= t0) return cg_fail(CG_EINVAL, std::string(fn) + ": t1 must lie after t0");
  AdmitCall adm;
  LockCall lk;
  if (admit)
    if (int rc = admit_units(fn, s, admit->dur_ms, admit->parallels, admit->unit, CG_PROFILE_DROPPED, t1 - t0, &adm))
      return rc;
  if (lock)
    if (int rc = lock_units(fn, s, lock->kind, lock->avg_time_ms, lock->unit, lock->contends, lock->lock_ttl,
                            CG_PROFILE_LOCK_SKIPPED, t1 - t0, &lk))
      return rc;
  // initial bytes: bit 0 for rules of units that can drop, bit 1 for contending
  // rules of lock units
  std::vector<uint8_t> flag(s->n, 0);
  for (size_t r = 0; r < s->n; r++)
    flag[r] = uint8_t((admit && adm.flag[r] ? kVerdictDropped : 0) | (lock && lk.flag[r] ? kVerdictSkipped : 0));
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  const int rc = verdicts_locked(c, s, z, t0, t1, admit ? &adm : nullptr, lock ? &lk : nullptr, flag, n_events);
  // adm, lk and flag are read by copies on the stream: a call that failed
  // between an upload and its synchronise drains the stream before they go
  if (rc) (void)hipStreamSynchronize(c->st);
  return rc;
}

int cg_verdicts_device(cg_ctx* c, const uint8_t** d_verdict, int64_t* n_events) {
  if (!c) return cg_fail(CG_EINVAL, "cg_verdicts_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  if (d_verdict) *d_verdict = c->vd_verdict.p;
  if (n_events) *n_events = c->vd_E;
  return CG_OK;
}

int cg_verdicts_copy(cg_ctx* c, int64_t first, int64_t count, uint8_t* out) {
  if (!c || (count > 0 && !out)) return cg_fail(CG_EINVAL, "cg_verdicts_copy: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  if (first < 0 || count < 0 || first > c->vd_E || count > c->vd_E - first)
    return cg_fail(CG_EINVAL, "range outside the last verdicts");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (count) HIPCHK(hipMemcpy(out, c->vd_verdict.p + first, size_t(count), hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_verdicts_select_device(cg_ctx* c, int mask, int value, int64_t* n_selected) {
  if (!c || !n_selected) return cg_fail(CG_EINVAL, "cg_verdicts_select_device: null");
  if (mask < 1 || mask > 3) return cg_fail(CG_EINVAL, "cg_verdicts_select_device: mask must be 1, 2 or 3");
  if (value & ~mask) return cg_fail(CG_EINVAL, "cg_verdicts_select_device: value has bits outside mask");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  c->vd_sel_valid = false;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_events(c->vdev))) return rc;
  hipStream_t st = c->st;
  const int64_t R = c->vd_R;
  c->vd_ms[4] = c->vd_ms[5] = 0.f;
  if ((rc = c->vd_sel_off.ensure(size_t(R) + 1)) || (rc = c->vd_sel_cnt.ensure(size_t(std::max<int64_t>(R, 1)))) ||
      (rc = c->scan_tmp.ensure(std::max(c->scan_tmp.cap, scan_temp_bytes(std::max<int64_t>(R, 1))))))
    return rc;
  int64_t n = 0;
  if (R == 0 || c->vd_E == 0) {
    HIPCHK(hipMemsetAsync(c->vd_sel_off.p, 0, (size_t(R) + 1) * 8, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = c->vd_sel_times.ensure(1))) return rc;
  } else {
    const int64_t* off = c->rs.offsets.p;
    (void)hipEventRecord(c->vdev[VDEV_SEL_COUNT], st);
    hipLaunchKernelGGL(k_verdict_count, dim3(gridn(R, 4, 1 << 16)), dim3(256), 0, st, off, R, c->vd_verdict.p,
                       uint32_t(mask), uint32_t(value), c->vd_sel_cnt.p);
    launch_scan(c->vd_sel_cnt.p, c->vd_sel_off.p, R, c->scan_tmp.p, st);
    (void)hipEventRecord(c->vdev[VDEV_SELECT], st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n, c->vd_sel_off.p + R, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&c->vd_ms[4], c->vdev[VDEV_SEL_COUNT], c->vdev[VDEV_SELECT]);
    if (n < 0 || n > c->vd_E) return cg_fail(CG_EHIP, "cg_verdicts_select_device: selection count out of range");
    if ((rc = c->vd_sel_times.ensure(size_t(std::max<int64_t>(n, 1))))) return rc;
    (void)hipEventRecord(c->vdev[VDEV_SELECT], st);
    if (n > 0)
      hipLaunchKernelGGL(k_verdict_select, dim3(gridn(R, 4, 1 << 16)), dim3(256), 0, st, off, R, c->vd_verdict.p,
                         c->times.p, uint32_t(mask), uint32_t(value), c->vd_sel_off.p, c->vd_sel_times.p);
    (void)hipEventRecord(c->vdev[VDEV_SELECT_END], st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&c->vd_ms[5], c->vdev[VDEV_SELECT], c->vdev[VDEV_SELECT_END]);
  }
  c->vd_nsel = n;
  c->vd_sel_valid = true;
  *n_selected = n;
  return CG_OK;
}

int cg_verdicts_selected_device(cg_ctx* c, const int64_t** d_sel_off, const int64_t** d_sel_times,
                                int64_t* n_selected) {
  if (!c) return cg_fail(CG_EINVAL, "cg_verdicts_selected_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  if (!c->vd_sel_valid) return no_selection();
  if (d_sel_off) *d_sel_off = c->vd_sel_off.p;
  if (d_sel_times) *d_sel_times = c->vd_sel_times.p;
  if (n_selected) *n_selected = c->vd_nsel;
  return CG_OK;
}

int cg_verdicts_selected_copy_offsets(cg_ctx* c, int64_t* out) {
  if (!c || !out) return cg_fail(CG_EINVAL, "cg_verdicts_selected_copy_offsets: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  if (!c->vd_sel_valid) return no_selection();
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(out, c->vd_sel_off.p, (size_t(c->vd_R) + 1) * 8, hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_verdicts_selected_copy_times(cg_ctx* c, int64_t first, int64_t count, int64_t* out) {
  if (!c || (count > 0 && !out)) return cg_fail(CG_EINVAL, "cg_verdicts_selected_copy_times: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!verdicts_readable(c)) return no_verdicts();
  if (!c->vd_sel_valid) return no_selection();
  if (first < 0 || count < 0 || first > c->vd_nsel || count > c->vd_nsel - first)
    return cg_fail(CG_EINVAL, "range outside the last selection");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (count) HIPCHK(hipMemcpy(out, c->vd_sel_times.p + first, size_t(count) * 8, hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_verdict_times(cg_ctx* c, float* ms, int n) {
  if (!c || (n > 0 && !ms)) return cg_fail(CG_EINVAL, "cg_verdict_times: null");
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < n && i < 6; i++) ms[i] = c->vd_ms[i];
  return n < 6 ? std::max(n, 0) : 6;
}

}  // extern "C"
