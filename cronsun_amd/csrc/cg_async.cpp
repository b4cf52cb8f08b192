// cg_async.cpp -- pipelined expansion for back-to-back calls (a scheduler's
// tick loop, SURVEY.md §8 a11: cron.go:212-215,242-243 batched per tick).
//
// A synchronous cg_expand_device ends every call with a stream sync (the
// caller reads the event total) and runs count -> scan -> write in series.
// cg_expand_device_async enqueues the same kernels and returns: the count and
// scan of call k run on a second stream, into a run set no queued writer
// reads (three sets), while call k-1's writer streams its output.  Call k's
// writer runs on writer stream k & 1 into output buffer k & 1 (the ctx stream
// and c->times, a second stream and c->times2): it follows call k-2's in
// stream order and shares nothing it writes with call k-1's, so the two are
// resident side by side (kWriteBlocksPerCUOverlap blocks per CU each) and the
// stores do not pause while one writer ends and the next starts.  Nothing on
// the device waits for another kernel.  Where the second buffer does not fit (or
// cg_set_async_overlap(0)) every writer runs on the ctx stream into c->times.
// The plan of each call (zone table, segments, day table) is staged through
// pinned memory of its run set, so a moving T0 costs no stream sync either.
// cg_expand_wait drains the pipeline and reports the calls' errors: a rule
// whose reference Next loop never ends (CG_ERANGE), or a result larger than
// the output capacity sized by an earlier synchronous call (CG_ECAPACITY: the
// writer then wrote nothing).
//
// The plan staging, count, scan and writers themselves are the run-set chain
// of cg_expand.cpp (run_set_count_scan / run_set_write_enqueue), the one the
// synchronous calls run on the ctx stream.  This file is the pipeline around
// it: which set, stream and output buffer a call gets (AsyncSet holds a
// RunSet and the bookkeeping of the call that last used it), the events that
// order and time the writers, and the checking of finished calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_kernels.h"
#include "cg_zone.h"

using namespace cg;

namespace {

// the record of a finished call on set a: fold its errors and writer time in
void check_set(cg_ctx* c, AsyncSet& a) {
  if (!a.pending) return;
  a.pending = false;
  // the call's writer time: start to end, or with the previous call's writer
  // on the other stream the part after that writer's end (the time to this
  // writer's completion not already counted for the previous call)
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->tw0[a.tslot], c->tw1[a.tslot]) == hipSuccess) {
    if (a.tprev >= 0) {
      float since_prev = 0.f;
      const hipError_t e = hipEventElapsedTime(&since_prev, c->tw1[a.tprev], c->tw1[a.tslot]);
      if (e == hipSuccess)
        ms = std::min(ms, std::max(since_prev, 0.f));
      else if (e == hipErrorNotReady)
        ms = 0.f;  // the previous writer is still running: it ends after this one
      (void)hipGetLastError();
    }
    c->wr_ms_sum += ms;
    c->wr_n++;
  }
  const int64_t E = a.rs.res_host[0];
  const unsigned long long stuck = static_cast<unsigned long long>(a.rs.res_host[1]);
  if (c->async_rc) return;  // keep the first error
  if (stuck != ~0ULL) {
    c->async_rc = CG_ERANGE;
    c->async_msg = stuck_msg(stuck);
  } else if (E > a.rs.cap) {
    c->async_rc = CG_ECAPACITY;
    c->async_msg = "async expansion: " + std::to_string(E) + " events exceed the output capacity " +
                   std::to_string(a.rs.cap) + " (run a synchronous cg_expand_device to grow it)";
  }
}

}  // namespace

int ensure_async(cg_ctx* c) {
  if (c->st_cs) return CG_OK;
  HIPCHK(hipStreamCreateWithFlags(&c->st_cs, hipStreamNonBlocking));
  for (hipEvent_t& e : c->cs_done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (AsyncSet& a : c->as) HIPCHK(hipEventCreateWithFlags(&a.written, hipEventDisableTiming));
  for (hipEvent_t* ring : {c->tw0, c->tw1})
    for (int i = 0; i < cg_ctx::kTimeRing; i++) HIPCHK(hipEventCreateWithFlags(&ring[i], hipEventDisableSystemFence));
  return CG_OK;
}

// A pipelined call made with nothing pending (both writer streams idle):
// whether the following calls alternate between two writer streams and output
// buffers.  The second buffer is taken only when cap events of it are at most
// half of the device memory free at this moment; where it does not fit, or its
// allocation fails, the calls run on the ctx stream into c->times alone.
static int overlap_decide(cg_ctx* c, int64_t cap) {
  c->ov_active = false;
  c->tw_prev = -1;
  if (c->st_w1 && c->w1_dirty) HIPCHK(hipStreamSynchronize(c->st_w1));
  c->w1_dirty = false;
  if (!c->ov_on) {
    c->times2.release();  // the caller's memory back
    return CG_OK;
  }
  if (!c->st_w1 && hipStreamCreateWithFlags(&c->st_w1, hipStreamNonBlocking) != hipSuccess) {
    c->st_w1 = nullptr;
    (void)hipGetLastError();
    return CG_OK;
  }
  if (int64_t(c->times2.cap) < cap) {  // a synchronous call grew c->times: follow it
    c->times2.release();
    size_t free_b = 0, total_b = 0;
    int64_t* p = nullptr;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || size_t(cap) * 8 > free_b / 2 ||
        hipMalloc(&p, size_t(cap) * 8) != hipSuccess) {
      (void)hipGetLastError();
      return CG_OK;
    }
    c->times2.p = p;
    c->times2.cap = size_t(cap);
  }
  c->ov_active = true;
  return CG_OK;
}

bool async_pending(const cg_ctx* c) {
  for (const AsyncSet& a : c->as)
    if (a.pending) return true;
  return false;
}

// every pending async call finished and checked (errors kept for the next wait)
int async_drain(cg_ctx* c) {
  bool any = false;
  for (const AsyncSet& a : c->as) any = any || a.pending;
  if (!any && !c->w1_dirty) return CG_OK;
  HIPCHK(hipStreamSynchronize(c->st));
  if (c->st_w1) HIPCHK(hipStreamSynchronize(c->st_w1));
  c->w1_dirty = false;
  for (AsyncSet& a : c->as) check_set(c, a);
  c->tw_prev = -1;  // the next call's writer starts on idle streams
  return CG_OK;
}

extern "C" {

int cg_expand_device_async(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1) {
  if (!c || !s || !z) return cg_fail(CG_EINVAL, "cg_expand_device_async: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (t1 - t0 > CG_MAX_HORIZON || t0 < -(int64_t(1) << 45) || t1 > (int64_t(1) << 45))
    return cg_fail(CG_ERANGE, "horizon must satisfy t1 - t0 <= CG_MAX_HORIZON (40 years)");
  const int64_t cap = int64_t(c->times.cap);
  if (cap == 0)
    return cg_fail(CG_ECAPACITY, "cg_expand_device_async: no output capacity yet (run cg_expand_device once)");
  int rc = ensure_async(c);
  if (rc) return rc;
  if (!async_pending(c) && (rc = overlap_decide(c, cap))) return rc;
  // this call's writer stream and output buffer
  const int wi = c->ov_active ? int(c->wr_call & 1) : 0;
  hipStream_t sw = wi ? c->st_w1 : c->st;
  int64_t* const out = wi ? c->times2.p : c->times.p;
  const int k = c->as_next;
  AsyncSet& a = c->as[k];
  // the set was last used kAsyncSets calls ago: its writer must be done
  // before the host restages its plan or the count stream rewrites its runs
  if (a.done) HIPCHK(hipEventSynchronize(a.done));
  check_set(c, a);
  a.done = nullptr;
  c->wr_call++;
  c->res_gen++;  // this call's writer replaces the readable result
  c->times_last = wi;
  if (wi) c->w1_dirty = true;
  const int64_t R = int64_t(s->n);
  bool empty = false;
  // count + scan on the second stream (the scan builds the writer's slice map
  // for the output capacity)
  if ((rc = run_set_count_scan(a.rs, s, z, t0, t1, cap, c->st_cs, nullptr, &empty))) return rc;
  if (empty) {  // nothing to count: zero offsets, an empty result
    HIPCHK(hipMemsetAsync(a.rs.offsets.p, 0, (R + 1) * 8, sw));
    c->as_next = (k + 1) % cg_ctx::kAsyncSets;
    c->as_last = k;
    c->last_R = R;
    c->last_E = 0;
    return CG_OK;
  }
  HIPCHK(hipEventRecord(c->cs_done[k], c->st_cs));
  // the writer after the last one on its stream, once this call's scan is done
  HIPCHK(hipStreamWaitEvent(sw, c->cs_done[k], 0));
  const bool has_walk = a.rs.has_walk();
  // with a writer of this batch possibly still running on the other stream the
  // two share the CUs: the smaller grid (the first writer after a drain runs
  // alone at its start and keeps the full one)
  const int blocks = c->ov_active && c->tw_prev >= 0 ? c->write_blocks_ov : c->write_blocks;
  a.tslot = c->tw_next;
  a.tprev = c->ov_active ? c->tw_prev : -1;
  c->tw_prev = a.tslot;
  c->tw_next = (a.tslot + 1) % cg_ctx::kTimeRing;
  (void)hipEventRecord(c->tw0[a.tslot], sw);
  run_set_write_enqueue(a.rs, s, cap, out, blocks, sw, c->tw1[a.tslot]);
  // the set is free again once its writer is done: without a walk that is the
  // end-of-writer event (one event packet fewer behind the writer; its ring
  // pair is re-recorded only after the set's next use has waited for it)
  a.done = c->tw1[a.tslot];
  if (has_walk) {
    HIPCHK(hipEventRecord(a.written, sw));
    a.done = a.written;
  }
  HIPCHK(hipGetLastError());
  a.pending = true;
  c->as_next = (k + 1) % cg_ctx::kAsyncSets;
  c->as_last = k;
  c->last_R = 0;  // nothing readable until cg_expand_wait (the accessors refuse while a call is pending)
  c->last_E = 0;
  return CG_OK;
}

int cg_expand_wait(cg_ctx* c, int64_t* n_events) {
  if (!c) return cg_fail(CG_EINVAL, "cg_expand_wait: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int rc = async_drain(c);
  if (rc) return rc;
  if (c->wr_n > 0) {
    c->kt[KT_X_WRITE_CF] = float(c->wr_ms_sum / c->wr_n);  // mean writer time of the calls checked (check_set)
    for (int i : {KT_X_COUNT, KT_X_SCAN, KT_X_MAP, KT_X_WRITE_WALK, KT_X_OFFSETS}) c->kt[i] = -1.f;
  }
  c->wr_ms_sum = 0;
  c->wr_n = 0;
  const int rc_async = c->async_rc;
  const std::string msg = c->async_msg;
  c->async_rc = 0;
  c->async_msg.clear();
  int64_t E = 0;
  if (c->as_last >= 0) {
    const RunSet& rs = c->as[c->as_last].rs;
    E = rs.res_host[0];
    c->last_E = rc_async ? 0 : E;
    c->last_R = rc_async ? 0 : rs.R;
  }
  if (n_events) *n_events = E;  // 0 when no asynchronous call was made since the last synchronous one
  if (rc_async) return cg_fail(rc_async, msg);
  return CG_OK;
}

int cg_set_async_overlap(cg_ctx* c, int on) {
  if (!c) return cg_fail(CG_EINVAL, "cg_set_async_overlap: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (async_pending(c))
    return cg_fail(CG_EINVAL, "cg_set_async_overlap: asynchronous expansions pending (call cg_expand_wait first)");
  c->ov_on = on != 0;
  return CG_OK;
}

}  // extern "C"
