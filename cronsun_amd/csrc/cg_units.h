// cg_units.h -- the host side of a unit walk, shared by cg_admit_* /
// cg_lock_profile_* (cg_profile.hip) and the fire verdicts (cg_verdict.hip):
// the checked per-rule arguments of an admission or a lock call, compacted into
// units; their upload; the LDS-budget refusals and the stuck-rule message.  Host
// only (the kernels' side is cg_unit_walk.h); the checks, their order, messages
// and codes are the same for every caller.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_admit.h"
#include "cg_api_internal.h"
#include "cg_lock.h"
#include "cg_profile.h"
#include "cg_unit_walk.h"

// An admission call's checked arguments: the units that can drop, compacted,
// and per rule whether its unit is one of them.  Host memory that outlives the
// stream synchronise that ends the call.
// RUNNING kinds also carry every rule's d (dsec, as an in-flight call's).
struct AdmitCall {
  int what = CG_PROFILE_ADMITTED;
  std::vector<cg::AdmitUnit> units;
  std::vector<uint8_t> flag;
  std::vector<int64_t> dsec;
  bool running() const { return what == CG_PROFILE_RUNNING; }
  const std::vector<int64_t>* durations() const { return running() ? &dsec : nullptr; }
};
// A lock call's: the lock units with a contending rule, compacted, and per
// rule whether it is a contending rule of a lock unit.
struct LockCall {
  int what = CG_PROFILE_LOCK_SKIPPED;
  int64_t lock_ttl = 0;
  std::vector<cg::LockUnit> units;
  std::vector<uint8_t> flag;
  std::vector<int64_t> dsec;
  bool running() const { return what == CG_PROFILE_LOCK_RUNNING; }
  const std::vector<int64_t>* durations() const { return running() ? &dsec : nullptr; }
};

// An admission call's per-rule arguments -> the units that can drop.  Units
// are the maximal runs of equal unit[] (NULL: every rule its own); all checks
// name the first offending rule.
inline int admit_units(const char* what_fn, const cg_specs* s, const int64_t* dur_ms, const int64_t* parallels,
                       const int32_t* unit, int what, int64_t horizon, AdmitCall* out) {
  using namespace cg;
  const std::string fn(what_fn);
  if (what != CG_PROFILE_ADMITTED && what != CG_PROFILE_DROPPED && what != CG_PROFILE_RUNNING)
    return cg_fail(CG_EINVAL, fn + ": what must be CG_PROFILE_ADMITTED, CG_PROFILE_DROPPED or CG_PROFILE_RUNNING");
  const int64_t R = int64_t(s->n);
  if (R > 0 && !dur_ms) return cg_fail(CG_EINVAL, fn + ": rule 0: null dur_ms");
  if (R > 0 && !parallels) return cg_fail(CG_EINVAL, fn + ": rule 0: null parallels");
  for (int64_t r = 0; r < R; r++) {
    if (dur_ms[r] < 0) return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r) + ": negative duration");
    if (parallels[r] < 0) return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r) + ": negative parallels");
    if (unit && r > 0 && unit[r] < unit[r - 1])
      return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r) + ": unit decreases");
  }
  out->what = what;
  out->units.clear();
  out->flag.assign(size_t(R), 0);
  out->dsec.clear();
  if (out->running()) {
    out->dsec.resize(size_t(R));
    for (int64_t r = 0; r < R; r++) out->dsec[size_t(r)] = inflight_seconds(dur_ms[r], horizon);
  }
  for (int64_t r0 = 0; r0 < R;) {
    int64_t r1 = r0 + 1;
    if (unit)
      for (; r1 < R && unit[r1] == unit[r0]; r1++)
        if (dur_ms[r1] != dur_ms[r0] || parallels[r1] != parallels[r0])
          return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r1) + ": dur_ms / parallels differ inside unit " +
                                        std::to_string(unit[r0]));
    const int64_t P = parallels[r0], d = inflight_seconds(dur_ms[r0], horizon), k = r1 - r0;
    if (!admit_never_drops(P, d, k)) {
      if (P > CG_ADMIT_MAX_PARALLELS)
        return cg_fail(CG_ERANGE, fn + ": rule " + std::to_string(r0) + ": parallels " + std::to_string(P) +
                                      " can drop and exceeds CG_ADMIT_MAX_PARALLELS (16)");
      if (k > INT32_MAX) return cg_fail(CG_ERANGE, fn + ": rule " + std::to_string(r0) + ": unit too long");
      out->units.push_back(AdmitUnit{r0, d, int32_t(k), int32_t(P)});
      for (int64_t r = r0; r < r1; r++) out->flag[size_t(r)] = 1;
    }
    r0 = r1;
  }
  return CG_OK;
}

// A lock call's per-rule arguments -> the lock units with a contending rule.
// Units are the maximal runs of equal unit[] (NULL: every rule its own); all
// checks name the first offending rule.
inline int lock_units(const char* what_fn, const cg_specs* s, const int32_t* kind, const int64_t* avg_ms,
                      const int32_t* unit, const uint8_t* contends, int64_t lock_ttl, int what, int64_t horizon,
                      LockCall* out) {
  using namespace cg;
  const std::string fn(what_fn);
  if (what != CG_PROFILE_LOCK_GRANTED && what != CG_PROFILE_LOCK_SKIPPED && what != CG_PROFILE_LOCK_RUNNING)
    return cg_fail(CG_EINVAL, fn + ": what must be CG_PROFILE_LOCK_GRANTED, CG_PROFILE_LOCK_SKIPPED or "
                                   "CG_PROFILE_LOCK_RUNNING");
  if (lock_ttl < 2) return cg_fail(CG_EINVAL, fn + ": lock_ttl must be at least 2 (conf.go:136-138)");
  const int64_t R = int64_t(s->n);
  if (R > 0 && !kind) return cg_fail(CG_EINVAL, fn + ": rule 0: null kind");
  if (R > 0 && !avg_ms) return cg_fail(CG_EINVAL, fn + ": rule 0: null avg_time_ms");
  for (int64_t r = 0; r < R; r++) {
    if (kind[r] != CG_JOB_COMMON && kind[r] != CG_JOB_ALONE && kind[r] != CG_JOB_INTERVAL)
      return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r) + ": kind " + std::to_string(kind[r]) +
                                    " is not CG_JOB_COMMON, CG_JOB_ALONE or CG_JOB_INTERVAL");
    if (unit && r > 0 && unit[r] < unit[r - 1])
      return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r) + ": unit decreases");
  }
  out->what = what;
  out->lock_ttl = lock_ttl;
  out->units.clear();
  out->flag.assign(size_t(R), 0);
  out->dsec.clear();
  if (out->running()) {
    out->dsec.resize(size_t(R));
    for (int64_t r = 0; r < R; r++)
      out->dsec[size_t(r)] = inflight_seconds(std::max<int64_t>(avg_ms[r], 0), horizon);
  }
  for (int64_t r0 = 0; r0 < R;) {
    int64_t r1 = r0 + 1;
    if (unit)
      for (; r1 < R && unit[r1] == unit[r0]; r1++)
        if (kind[r1] != kind[r0] || avg_ms[r1] != avg_ms[r0])
          return cg_fail(CG_EINVAL, fn + ": rule " + std::to_string(r1) + ": kind / avg_time_ms differ inside unit " +
                                        std::to_string(unit[r0]));
    if (kind[r0] != CG_JOB_COMMON) {
      if (r1 - r0 > INT32_MAX) return cg_fail(CG_ERANGE, fn + ": rule " + std::to_string(r0) + ": unit too long");
      bool any = false;
      for (int64_t r = r0; r < r1; r++)
        if (!contends || contends[r]) any = true, out->flag[size_t(r)] = 1;
      if (any)
        out->units.push_back(LockUnit{r0, avg_ms[r0], inflight_seconds(std::max<int64_t>(avg_ms[r0], 0), horizon),
                                      int32_t(r1 - r0), kind[r0]});
    }
    r0 = r1;
  }
  return CG_OK;
}

// Uploads a call's units and flags into the ctx's shared buffers (uw_*, slot 0
// admission, slot 1 lock; adm / lk null: none of that kind) on the ctx stream
// and, with err, sets both error words to ~0.  flag0: slot 0's flags when they
// are not adm's own (a verdict call's initial bytes).  The host arrays must
// outlive the stream synchronise that ends the call; c->mu held.
inline int unit_upload(cg_ctx* c, int64_t R, const AdmitCall* adm, const LockCall* lk, const uint8_t* flag0,
                       bool err) {
  using namespace cg;
  static_assert(sizeof(AdmitUnit) == 24 && sizeof(LockUnit) == 32, "units are uploaded as packed records");
  hipStream_t st = c->st;
  int rc;
  if (adm && !flag0) flag0 = adm->flag.data();
  if (flag0) {
    if ((rc = c->uw_flag[0].ensure(size_t(R)))) return rc;
    HIPCHK(hipMemcpyAsync(c->uw_flag[0].p, flag0, size_t(R), hipMemcpyHostToDevice, st));
  }
  if (adm) {
    const size_t bytes = adm->units.size() * sizeof(AdmitUnit);
    if ((rc = c->uw_units[0].ensure(std::max<size_t>(bytes, 1)))) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(c->uw_units[0].p, adm->units.data(), bytes, hipMemcpyHostToDevice, st));
  }
  if (lk) {
    const size_t bytes = lk->units.size() * sizeof(LockUnit);
    if ((rc = c->uw_flag[1].ensure(size_t(R))) || (rc = c->uw_units[1].ensure(std::max<size_t>(bytes, 1)))) return rc;
    HIPCHK(hipMemcpyAsync(c->uw_flag[1].p, lk->flag.data(), size_t(R), hipMemcpyHostToDevice, st));
    if (bytes) HIPCHK(hipMemcpyAsync(c->uw_units[1].p, lk->units.data(), bytes, hipMemcpyHostToDevice, st));
  }
  if (err) {
    if ((rc = c->uw_err.ensure(2))) return rc;
    HIPCHK(hipMemsetAsync(c->uw_err.p, 0xFF, 2 * sizeof(unsigned long long), st));
  }
  return CG_OK;
}
inline const cg::AdmitUnit* uw_admit_units(const cg_ctx* c) {
  return reinterpret_cast<const cg::AdmitUnit*>(c->uw_units[0].p);
}
inline const cg::LockUnit* uw_lock_units(const cg_ctx* c) {
  return reinterpret_cast<const cg::LockUnit*>(c->uw_units[1].p);
}

// the error words behind the walks: copied back, the stream drained
inline int unit_errors(cg_ctx* c, unsigned long long err[2]) {
  err[0] = err[1] = ~0ULL;
  HIPCHK(hipMemcpyAsync(err, c->uw_err.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

// a walk's launch must fit the 64 KiB of LDS behind the staged plan
inline int admit_lds_check(const char* fn, size_t plan_lds) {
  if (cg::admit_lds_bytes(plan_lds) <= 64 * 1024) return CG_OK;
  return cg_fail(CG_ERANGE, std::string(fn) + ": the plan of this horizon leaves no LDS for the admission ring");
}
inline int lock_lds_check(const char* fn, size_t plan_lds) {
  if (cg::lock_lds_bytes(plan_lds) <= 64 * 1024) return CG_OK;
  return cg_fail(CG_ERANGE,
                 std::string(fn) + ": the plan of this horizon leaves no LDS for the walked runs' positions");
}
// a granted fire whose Next never returns: the reference hangs in lockTtl
// there, and the unit's rows or bytes are unfinished
inline std::string lock_stuck_msg(const char* fn, unsigned long long rule) {
  return std::string(fn) + ": rule " + std::to_string(rule) +
         ": Next never returns from a fire of this horizon that finds the lock free "
         "(the reference's lockTtl does not return there)";
}
