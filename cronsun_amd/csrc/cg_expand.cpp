// cg_expand.cpp -- the rule-major expansion: the run-set chain (plan, count,
// scan, writers) every expansion entry point runs, the synchronous entry
// points cg_count / cg_expand_device / cg_expand and the result accessors.
// The pipelined entry points (cg_async.cpp, cg_pernode.hip) enqueue the same
// chain on their own run sets and streams.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_kernels.h"
#include "cg_zone.h"

using namespace cg;

// ------------------------------------------------------------ run-set chain
int run_set_count_scan(RunSet& rs, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1, int64_t map_cap,
                       hipStream_t st, hipEvent_t* ev, bool* empty, bool lock_table) {
  int rc;
  const int64_t R = int64_t(s->n);
  if ((rc = rs.ensure_res())) return rc;
  // plan (cached across identical calls): packed into the pinned buffer here,
  // copied once every allocation below has succeeded
  const bool fresh = !(rs.plan_valid && rs.plan_zone == z->serial && rs.plan_t0 == t0 && rs.plan_t1 == t1 &&
                       rs.plan_lock_table == lock_table);
  PlanLayout L{};
  if (fresh) {
    rs.plan_valid = false;
    rs.plan = build_plan(z->rules, t0, t1);
    // a lock profile's Next calls read past the horizon's table (cg_zone.h)
    if (lock_table) rs.plan.table = build_lock_table(z->rules, t0, t1);
    L = plan_layout(rs.plan);
    if (rs.plan_pin_cap < L.bytes) {
      if (rs.plan_pin) (void)hipHostFree(rs.plan_pin);
      rs.plan_pin = nullptr;
      rs.plan_pin_cap = 0;
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&rs.plan_pin), L.bytes));
      rs.plan_pin_cap = L.bytes;
    }
    plan_pack(rs.plan, L, rs.plan_pin);
    if ((rc = rs.plan_dev.ensure(L.bytes))) return rc;
    if ((rc = plan_args(rs.plan, L, rs.plan_dev.p, t0, t1, &rs.pa))) return rc;
  }
  const PlanArgs& pa = rs.pa;
  const int64_t G = pa.G, nruns = R * G;
  *empty = nruns == 0;
  if ((rc = rs.offsets.ensure(R + 1))) return rc;
  if (!*empty &&
      ((rc = rs.run_anchor.ensure(nruns)) || (rc = rs.run_count.ensure(nruns)) || (rc = rs.run_dmask.ensure(nruns)) ||
       (rc = rs.run_off.ensure(nruns + 1)) || (rc = rs.scan_tmp.ensure(scan_temp_bytes(nruns))) ||
       (map_cap > 0 && (rc = rs.block_run.ensure(slice_map_words(map_cap)))) || (rc = rs.stuck.ensure(1))))
    return rc;
  if (fresh) {
    HIPCHK(hipMemcpyAsync(rs.plan_dev.p, rs.plan_pin, L.bytes, hipMemcpyHostToDevice, st));
    rs.plan_valid = true;
    rs.plan_zone = z->serial;
    rs.plan_t0 = t0;
    rs.plan_t1 = t1;
    rs.plan_lock_table = lock_table;
  }
  rs.R = R;
  rs.cap = map_cap;
  if (*empty) {
    rs.res_host[0] = 0;
    rs.res_host[1] = -1;
    return CG_OK;
  }
  if (!rs.armed) HIPCHK(hipMemsetAsync(rs.stuck.p, 0xFF, sizeof(unsigned long long), st));
  rs.armed = true;  // see RunSet::armed
  if (ev) (void)hipEventRecord(ev[0], st);
  launch_count(s->d, R, pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, rs.stuck.p, st);
  if (ev) (void)hipEventRecord(ev[1], st);
  launch_scan_runs(rs.run_count.p, rs.run_off.p, R, int32_t(G), rs.scan_tmp.p, rs.offsets.p, rs.res_dev, rs.stuck.p,
                   map_cap > 0 ? rs.block_run.p : nullptr, map_cap, st);
  if (ev) (void)hipEventRecord(ev[2], st);
  HIPCHK(hipGetLastError());
  return CG_OK;
}

void run_set_write_enqueue(const RunSet& rs, const cg_specs* s, int64_t cap, int64_t* out, int blocks,
                           hipStream_t st, hipEvent_t after_cf) {
  launch_write_cf(s->d, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, rs.run_off.p, rs.R * int64_t(rs.pa.G),
                  rs.block_run.p, cap, out, blocks, st);
  if (after_cf) (void)hipEventRecord(after_cf, st);
  if (rs.has_walk())
    launch_write_walk(s->d, rs.R, rs.pa, rs.run_anchor.p, rs.run_count.p, rs.run_dmask.p, rs.run_off.p, cap, out, st);
}

std::string stuck_msg(unsigned long long rule) {
  return "rule " + std::to_string(rule) +
         ": the reference Next loop never terminates inside this horizon "
         "(Next does not return, or returns a time <= its input and cycles)";
}

// ------------------------------------------------------- synchronous calls
// What a synchronous call does before its count and scan on the ctx stream
// into c->rs; an empty call's offsets are zeroed and the stream drained.
int sync_count_scan(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1, bool* empty,
                    int64_t map_cap, bool lock_table) {
  // no readable result until this call succeeds (the accessors check last_R/E).
  // Asynchronous calls still pending are drained and their results and errors
  // discarded: this call's result replaces them (cronsun_gpu.h).
  int rc0 = async_drain(c);
  if (rc0) return rc0;
  c->async_rc = 0;
  c->async_msg.clear();
  if ((rc0 = pn_async_drain(c))) return rc0;  // the same for pipelined per-node windows
  c->pa_rc = 0;
  c->pa_msg.clear();
  c->pa_last = -1;
  c->pa_en_sum = 0;
  c->as_last = -1;
  c->times_last = 0;  // synchronous calls write c->times
  c->last_R = 0;
  c->last_E = 0;
  c->res_gen++;  // verdicts and selections of the replaced result go stale
  HIPCHK(hipSetDevice(c->device));
  if (t1 - t0 > CG_MAX_HORIZON || t0 < -(int64_t(1) << 45) || t1 > (int64_t(1) << 45))
    return cg_fail(CG_ERANGE, "horizon must satisfy t1 - t0 <= CG_MAX_HORIZON (40 years)");
  for (int i = KT_X_COUNT; i <= KT_X_OFFSETS; i++) c->kt[i] = 0;
  int rc = run_set_count_scan(c->rs, s, z, t0, t1, map_cap, c->st, c->phase_timing >= 2 ? c->ev : nullptr, empty,
                              lock_table);
  if (rc) return rc;
  if (*empty) {
    HIPCHK(hipMemsetAsync(c->rs.offsets.p, 0, (int64_t(s->n) + 1) * 8, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  return CG_OK;
}

static int stuck_error(unsigned long long stuck) { return cg_fail(CG_ERANGE, stuck_msg(stuck)); }

int expand_device_locked(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                         int64_t* n_events, bool lock_table) {
  bool empty = true;
  // steady state: the output buffer exists, so the scan builds the writer's
  // slice map for its capacity (a first or a growing call maps separately)
  const int64_t cap0 = int64_t(c->times.cap);
  int rc = sync_count_scan(c, s, z, t0, t1, &empty, cap0, lock_table);
  if (rc) return rc;
  const int64_t R = int64_t(s->n);
  if (empty) {
    c->last_R = R;  // offsets are all zero
    c->last_E = 0;
    *n_events = 0;
    return CG_OK;
  }
  RunSet& rs = c->rs;
  const int64_t nruns = R * int64_t(rs.pa.G);
  // Write phase without a host round trip: the chunk map and writers read the
  // event total from device memory and size their work from it.  Output
  // capacity comes from earlier calls; the first call (or a larger result)
  // syncs once to size the buffers and relaunches the write phase.
  if (c->times.cap == 0) {
    int64_t E0 = 0;
    HIPCHK(hipMemcpyAsync(&E0, rs.run_off.p + nruns, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if ((rc = c->times.ensure(std::max<int64_t>(E0, 1)))) return rc;
  }
  const bool all_phases = c->phase_timing >= 2;
  int64_t E = 0;
  unsigned long long stuck = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    const int64_t cap = int64_t(c->times.cap);
    if ((rc = rs.block_run.ensure(slice_map_words(cap)))) return rc;
    if (all_phases) (void)hipEventRecord(c->ev[3], c->st);
    if (!(cap0 > 0 && cap == cap0))
      launch_chunk_map(rs.run_off.p, nruns, cap, rs.block_run.p, c->st);
    (void)hipEventRecord(c->ev[4], c->st);
    run_set_write_enqueue(rs, s, cap, c->times.p, c->write_blocks, c->st, c->ev[5]);
    if (all_phases) (void)hipEventRecord(c->ev[6], c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    E = rs.res_host[0];
    stuck = static_cast<unsigned long long>(rs.res_host[1]);
    if (stuck != ~0ULL) return stuck_error(stuck);
    if (E <= cap) break;
    if ((rc = c->times.ensure(E))) return rc;  // grow and redo the write phase
  }
  (void)hipEventElapsedTime(&c->kt[KT_X_WRITE_CF], c->ev[4], c->ev[5]);
  if (all_phases) {
    (void)hipEventElapsedTime(&c->kt[KT_X_COUNT], c->ev[0], c->ev[1]);
    (void)hipEventElapsedTime(&c->kt[KT_X_SCAN], c->ev[1], c->ev[2]);
    (void)hipEventElapsedTime(&c->kt[KT_X_MAP], c->ev[3], c->ev[4]);
    (void)hipEventElapsedTime(&c->kt[KT_X_WRITE_WALK], c->ev[5], c->ev[6]);
    c->kt[KT_X_OFFSETS] = 0.f;  // per-rule offsets: written by the scan (k_scan_apply)
  } else {
    c->kt[KT_X_COUNT] = c->kt[KT_X_SCAN] = c->kt[KT_X_MAP] = c->kt[KT_X_WRITE_WALK] = c->kt[KT_X_OFFSETS] = -1.f;
  }
  c->last_R = R;
  c->last_E = E;
  *n_events = E;
  return CG_OK;
}

extern "C" int cg_count(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                        int64_t* counts, int64_t* total) {
  if (!c || !s || !z || !total || (s->n && !counts)) return cg_fail(CG_EINVAL, "cg_count: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  bool empty = true;
  int rc = sync_count_scan(c, s, z, t0, t1, &empty);
  if (rc) return rc;
  const int64_t R = int64_t(s->n);
  if (empty) {
    for (int64_t r = 0; r < R; r++) counts[r] = 0;
    *total = 0;
    return CG_OK;
  }
  HIPCHK(hipGetLastError());
  std::vector<int64_t> off(size_t(R) + 1);
  HIPCHK(hipMemcpyAsync(off.data(), c->rs.offsets.p, (R + 1) * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  const unsigned long long stuck = static_cast<unsigned long long>(c->rs.res_host[1]);
  if (stuck != ~0ULL) return stuck_error(stuck);
  for (int64_t r = 0; r < R; r++) counts[r] = off[size_t(r) + 1] - off[size_t(r)];
  *total = off[size_t(R)];
  return CG_OK;  // (no expansion result to read after a count: last_R = last_E = 0)
}

extern "C" {

int cg_expand_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                     int64_t* n_events) {
  if (!c || !s || !z || !n_events) return cg_fail(CG_EINVAL, "cg_expand_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  return expand_device_locked(c, s, z, t0, t1, n_events);
}

int cg_expand(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
              cg_csr* out) {
  if (!c || !s || !z || !out) return cg_fail(CG_EINVAL, "cg_expand: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  int64_t E = 0;
  int rc = expand_device_locked(c, s, z, t0, t1, &E);
  if (rc) return rc;
  out->n_events = E;
  if (out->offsets)
    HIPCHK(hipMemcpy(out->offsets, c->rs.offsets.p, (s->n + 1) * 8, hipMemcpyDeviceToHost));
  if (out->times) {
    if (out->times_cap < E) return cg_fail(CG_ECAPACITY, "times buffer too small; see n_events");
    if (E) HIPCHK(hipMemcpy(out->times, c->times.p, E * 8, hipMemcpyDeviceToHost));
  }
  return CG_OK;
}

// ------------------------------------------------------- result accessors
static int refuse_pending(cg_ctx* c, const char* what) {
  if (!async_pending(c)) return CG_OK;
  return cg_fail(CG_EINVAL, std::string(what) + ": asynchronous expansions pending (call cg_expand_wait first)");
}

// the rule offsets of the last result: of the last pipelined call's set, or
// the synchronous set's
static const int64_t* result_offsets(const cg_ctx* c) {
  return c->as_last >= 0 ? c->as[c->as_last].rs.offsets.p : c->rs.offsets.p;
}

int cg_result_device(cg_ctx* c, const int64_t** d_off, const int64_t** d_times, int64_t* n) {
  if (!c) return cg_fail(CG_EINVAL, "cg_result_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = refuse_pending(c, "cg_result_device")) return rc;
  if (d_off) *d_off = result_offsets(c);
  if (d_times) *d_times = c->result_times();
  if (n) *n = c->last_E;
  return CG_OK;
}

int cg_result_copy_times(cg_ctx* c, int64_t first, int64_t count, int64_t* host) {
  if (!c || (count && !host)) return cg_fail(CG_EINVAL, "cg_result_copy_times: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = refuse_pending(c, "cg_result_copy_times")) return rc;
  if (first < 0 || count < 0 || first + count > c->last_E)
    return cg_fail(CG_EINVAL, "range outside the last result");
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  HIPCHK(hipSetDevice(c->device));
  if (count) HIPCHK(hipMemcpy(host, c->result_times() + first, count * 8, hipMemcpyDeviceToHost));
  return CG_OK;
}

int cg_result_copy_offsets(cg_ctx* c, int64_t* host) {
  if (!c || !host) return cg_fail(CG_EINVAL, "cg_result_copy_offsets: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = refuse_pending(c, "cg_result_copy_offsets")) return rc;
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(host, result_offsets(c), (c->last_R + 1) * 8, hipMemcpyDeviceToHost));
  return CG_OK;
}

}  // extern "C"
