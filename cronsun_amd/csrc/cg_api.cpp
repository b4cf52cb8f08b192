// cg_api.cpp -- the C-ABI of include/cronsun_gpu.h: contexts, device memory,
// zones, spec upload, plan packing, Next and lockTtl batches and the device
// utilities (the expansion is cg_expand.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_kernels.h"
#include "cg_parse.h"
#include "cg_zone.h"

using namespace cg;

namespace {
thread_local std::string g_err;
}

int cg_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int cg_hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return CG_OK;
  return cg_fail(e == hipErrorOutOfMemory ? CG_ENOMEM : CG_EHIP,
                 std::string(what) + ": " + hipGetErrorString(e));
}



static uint64_t next_serial() {
  static std::mutex m;
  static uint64_t s = 0;
  std::lock_guard<std::mutex> g(m);
  return ++s;
}

extern "C" {

int cg_abi_version(void) { return CG_ABI_VERSION; }

const char* cg_last_error(void) { return g_err.c_str(); }

int cg_build_info(void) {
#ifdef CG_DIAG
  return CG_BUILD_DIAG;
#else
  return 0;
#endif
}

int cg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; i++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) != hipSuccess) continue;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ok++;
  }
  return ok;
}

// ------------------------------------------------------------------ zones
int cg_zone_from_tzif(const uint8_t* data, size_t len, cg_zone** out) {
  if (!data || !out) return cg_fail(CG_EINVAL, "cg_zone_from_tzif: null");
  ZoneRules r;
  std::string e;
  if (!zone_from_tzif(data, len, &r, &e)) return cg_fail(CG_EINVAL, "TZif: " + e);
  *out = new cg_zone{std::move(r), next_serial()};
  return CG_OK;
}

int cg_zone_fixed(int32_t off, cg_zone** out) {
  if (!out) return cg_fail(CG_EINVAL, "cg_zone_fixed: null");
  *out = new cg_zone{zone_fixed(off), next_serial()};
  return CG_OK;
}

int cg_zone_utc(cg_zone** out) {
  if (!out) return cg_fail(CG_EINVAL, "cg_zone_utc: null");
  *out = new cg_zone{zone_utc(), next_serial()};
  return CG_OK;
}

void cg_zone_free(cg_zone* z) { delete z; }

int cg_zone_offset(const cg_zone* z, int64_t t, int32_t* off) {
  if (!z || !off) return cg_fail(CG_EINVAL, "cg_zone_offset: null");
  *off = z->rules.offset(t);
  return CG_OK;
}

int cg_zone_table(const cg_zone* z, int64_t lo, int64_t hi, int64_t* when, int32_t* off, int cap) {
  if (!z) return cg_fail(CG_EINVAL, "cg_zone_table: null");
  ZoneTable t = build_table(z->rules, lo, hi);
  int n = int(t.when.size());
  for (int i = 0; i < n && i < cap; i++) {
    if (when) when[i] = t.when[i];
    if (off) off[i] = t.off[i];
  }
  return n;
}

// ---------------------------------------------------------------- context
int cg_init(int device, cg_ctx** out) {
  if (!out) return cg_fail(CG_EINVAL, "cg_init: null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return cg_fail(CG_ENODEV, "no HIP device visible (this engine has no CPU fallback)");
  if (device < 0 || device >= n) return cg_fail(CG_ENODEV, "device index out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return cg_fail(CG_ENODEV, std::string("device is ") + prop.gcnArchName + ", need gfx950");
  HIPCHK(hipSetDevice(device));
  cg_ctx* c = new cg_ctx();
  c->device = device;
  int per_cu = kWriteBlocksPerCU;
#ifdef CG_DIAG
  if (const char* e = getenv("CG_WRITE_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(e));
#endif
  c->write_blocks = std::max(1, prop.multiProcessorCount) * per_cu;
  c->write_blocks_ov = std::max(1, prop.multiProcessorCount) * std::min(per_cu, kWriteBlocksPerCUOverlap);
  if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return cg_fail(CG_EHIP, "hipStreamCreate failed");
  }
  // timing-only events (read after a stream sync): no system-scope fence
  // when they complete -- a fenced event between two kernels idles the GPU
  // for several us (cache writeback + invalidate)
  for (auto& e : c->ev) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  for (auto& e : c->pev) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  *out = c;
  return CG_OK;
}

void cg_destroy(cg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->st);
  if (c->st_cs) (void)hipStreamSynchronize(c->st_cs);
  if (c->st_w1) (void)hipStreamSynchronize(c->st_w1);
  c->free_all();
  for (auto& e : c->ev) (void)hipEventDestroy(e);
  for (auto& e : c->pev) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->st);
  delete c;
}

int cg_sync(cg_ctx* c) {
  if (!c) return cg_fail(CG_EINVAL, "cg_sync: null");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->st));
  if (c->st_w1) HIPCHK(hipStreamSynchronize(c->st_w1));  // the pipelined path's second writer stream
  return CG_OK;
}

// ------------------------------------------------------------------ specs
}  // extern "C"

int pack_spec(const cg_schedule& s, DSpec* d) {
  std::memset(d, 0, sizeof *d);
  if (s.kind == 1) {
    if (s.delay_ns <= 0 || s.delay_ns % 1000000000LL != 0)
      return cg_fail(CG_EINVAL,
                     "ConstantDelaySchedule.Delay must be a positive whole number of seconds "
                     "(cron.Every guarantees this)");
    d->kind = KIND_EVERY;
    d->sec = uint64_t(s.delay_ns / 1000000000LL);
    return CG_OK;
  }
  if (s.kind != 0) return cg_fail(CG_EINVAL, "unknown schedule kind");
  d->kind = KIND_SPEC;
  d->sec = s.second & 0x0FFFFFFFFFFFFFFFull;
  d->min = s.minute & 0x0FFFFFFFFFFFFFFFull;
  d->hour = uint32_t(s.hour & 0xFFFFFFu);
  d->dom = uint32_t(s.dom & 0xFFFFFFFEu) | uint32_t((s.dom >> 63) & 1u);
  d->mondow = uint32_t(s.month & 0x1FFEu) | (uint32_t(s.dow & 0x7Fu) << 16) |
              (uint32_t((s.dow >> 63) & 1u) << 23);
  return CG_OK;
}

extern "C" {

static int upload_packed(cg_ctx* c, const std::vector<DSpec>& h, cg_specs** out) {
  HIPCHK(hipSetDevice(c->device));
  cg_specs* s = new cg_specs();
  s->ctx = c;
  s->n = h.size();
  s->owner = true;
  if (!h.empty()) {
    hipError_t e = hipMalloc(&s->d, h.size() * sizeof(DSpec));
    if (e != hipSuccess) {
      delete s;
      return cg_hip_check(e, "hipMalloc(specs)");
    }
    e = hipMemcpy(s->d, h.data(), h.size() * sizeof(DSpec), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(s->d);
      delete s;
      return cg_hip_check(e, "hipMemcpy(specs)");
    }
  }
  *out = s;
  return CG_OK;
}

int cg_specs_upload(cg_ctx* c, const cg_spec_soa* soa, size_t n, cg_specs** out) {
  if (!c || !soa || !out) return cg_fail(CG_EINVAL, "cg_specs_upload: null");
  std::vector<DSpec> h(n);
  for (size_t i = 0; i < n; i++) {
    cg_schedule s;
    std::memset(&s, 0, sizeof s);
    if (soa->delay_ns && soa->delay_ns[i] > 0) {
      s.kind = 1;
      s.delay_ns = soa->delay_ns[i];
    } else {
      s.second = soa->second ? soa->second[i] : 0;
      s.minute = soa->minute ? soa->minute[i] : 0;
      s.hour = soa->hour ? soa->hour[i] : 0;
      s.dom = soa->dom ? soa->dom[i] : 0;
      s.month = soa->month ? soa->month[i] : 0;
      s.dow = soa->dow ? soa->dow[i] : 0;
    }
    int rc = pack_spec(s, &h[i]);
    if (rc) return rc;
  }
  return upload_packed(c, h, out);
}

int cg_specs_upload_schedules(cg_ctx* c, const cg_schedule* s, size_t n, cg_specs** out) {
  if (!c || (!s && n) || !out) return cg_fail(CG_EINVAL, "cg_specs_upload_schedules: null");
  std::vector<DSpec> h(n);
  for (size_t i = 0; i < n; i++) {
    int rc = pack_spec(s[i], &h[i]);
    if (rc) return rc;
  }
  return upload_packed(c, h, out);
}

int cg_specs_slice(cg_specs* p, size_t first, size_t count, cg_specs** out) {
  if (!p || !out) return cg_fail(CG_EINVAL, "cg_specs_slice: null");
  if (first > p->n || count > p->n - first) return cg_fail(CG_EINVAL, "slice out of range");
  cg_specs* s = new cg_specs();
  s->ctx = p->ctx;
  s->d = p->d + first;
  s->n = count;
  s->owner = false;
  *out = s;
  return CG_OK;
}

size_t cg_specs_count(const cg_specs* s) { return s ? s->n : 0; }

void cg_specs_free(cg_specs* s) {
  if (!s) return;
  if (s->owner && s->d) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipFree(s->d);
  }
  delete s;
}

}  // extern "C"

// ----------------------------------------------------------- plan packing
// one packed upload: when | off | segs | dtab
PlanLayout plan_layout(const Plan& plan) {
  PlanLayout L;
  const size_t zn = plan.table.when.size(), G = plan.segs.size(), nd = plan.dtab.size();
  L.o_when = 0;
  L.o_off = L.o_when + zn * 8;
  L.o_seg = (L.o_off + zn * 4 + 15) / 16 * 16;
  L.o_dt = L.o_seg + G * sizeof(Segment);
  L.bytes = L.o_dt + nd * 4 + 16;
  return L;
}

void plan_pack(const Plan& plan, const PlanLayout& L, char* h) {
  std::memset(h, 0, L.bytes);
  std::memcpy(h + L.o_when, plan.table.when.data(), plan.table.when.size() * 8);
  std::memcpy(h + L.o_off, plan.table.off.data(), plan.table.off.size() * 4);
  if (!plan.segs.empty()) std::memcpy(h + L.o_seg, plan.segs.data(), plan.segs.size() * sizeof(Segment));
  if (!plan.dtab.empty()) std::memcpy(h + L.o_dt, plan.dtab.data(), plan.dtab.size() * 4);
}

int plan_args(const Plan& plan, const PlanLayout& L, char* base, int64_t t0, int64_t t1, PlanArgs* pa) {
  const int32_t G = int32_t(plan.segs.size());
  if (G > kMaxSegments)
    return cg_fail(CG_ERANGE, "plan has more than " + std::to_string(kMaxSegments) +
                                  " segments (horizon too long for this zone)");
  pa->zwhen = reinterpret_cast<const int64_t*>(base + L.o_when);
  pa->zoff = reinterpret_cast<const int32_t*>(base + L.o_off);
  pa->segs = reinterpret_cast<const Segment*>(base + L.o_seg);
  pa->dtab = reinterpret_cast<const uint32_t*>(base + L.o_dt);
  pa->zn = int32_t(plan.table.when.size());
  pa->G = G;
  pa->nd = int32_t(plan.dtab.size());
  pa->dtab_global = 0;
  pa->flags = plan.flags;
  pa->t0 = t0;
  pa->t1 = t1;
  // long horizons: the day table (4 B per local day) stays in HBM and the
  // zone table + segments alone are staged
  if (plan_lds_bytes(*pa) > kPlanLdsBytes) pa->dtab_global = 1;
  if (plan_lds_bytes(*pa) > kPlanLdsBytes)
    return cg_fail(CG_ERANGE, "zone table too large for LDS staging (narrow the time range)");
  return CG_OK;
}

// the plan of a Next / lockTtl batch into the ctx's plan_dev (an expansion
// stages its own into its run set, cg_expand.cpp)
int upload_plan(cg_ctx* c, const Plan& plan, int64_t t0, int64_t t1, PlanArgs* pa) {
  if (plan.segs.size() > size_t(kMaxSegments))
    return cg_fail(CG_ERANGE, "plan has more than " + std::to_string(kMaxSegments) +
                                  " segments (horizon too long for this zone)");
  const PlanLayout L = plan_layout(plan);
  std::vector<char>& h = c->plan_host;
  h.assign(L.bytes, 0);
  plan_pack(plan, L, h.data());
  int rc = c->plan_dev.ensure(L.bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->plan_dev.p, h.data(), L.bytes, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));  // h is reused by the next call
  return plan_args(plan, L, c->plan_dev.p, t0, t1, pa);
}

extern "C" {

// ------------------------------------------------------------------ Next()
int cg_next_batch(cg_ctx* c, const cg_specs* s, const cg_zone* z, const int64_t* t_in,
                  int64_t* t_out) {
  if (!c || !s || !z || (s->n && (!t_in || !t_out))) return cg_fail(CG_EINVAL, "cg_next_batch: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  HIPCHK(hipSetDevice(c->device));
  const int64_t n = int64_t(s->n);
  if (n == 0) return CG_OK;
  int64_t lo = t_in[0], hi = t_in[0];
  for (int64_t i = 1; i < n; i++) {
    lo = std::min(lo, t_in[i]);
    hi = std::max(hi, t_in[i]);
  }
  const int64_t kDay = 86400;
  if (lo < -(int64_t(1) << 45) || hi > (int64_t(1) << 45))
    return cg_fail(CG_ERANGE, "input time outside +-1.1M years");
  Plan plan;
  // Next walks back to the month start of t+1 and forward at most ~6 years
  plan.table = build_table(z->rules, lo - 64 * kDay, hi + (6 * 366 + 64) * kDay);
  PlanArgs pa;
  int rc = upload_plan(c, plan, 0, 0, &pa);
  if (rc) return rc;
  if ((rc = c->nb_in.ensure(n))) return rc;
  if ((rc = c->nb_out.ensure(n))) return rc;
  HIPCHK(hipMemcpyAsync(c->nb_in.p, t_in, n * 8, hipMemcpyHostToDevice, c->st));
  launch_next_batch(s->d, n, pa, c->nb_in.p, c->nb_out.p, c->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t_out, c->nb_out.p, n * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

// ---------------------------------------------------------- Cmd.lockTtl()
int cg_lock_ttl_batch(cg_ctx* c, const cg_specs* s, const cg_zone* z, const int64_t* now,
                      const int32_t* kind, const int64_t* avg_time_ms, int64_t lock_ttl,
                      int64_t* ttl_out) {
  if (!c || !s || !z || (s->n && (!now || !kind || !avg_time_ms || !ttl_out)))
    return cg_fail(CG_EINVAL, "cg_lock_ttl_batch: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  const int64_t n = int64_t(s->n);
  if (n == 0) return CG_OK;
  int64_t lo = now[0], hi = now[0];
  for (int64_t i = 1; i < n; i++) {
    lo = std::min(lo, now[i]);
    hi = std::max(hi, now[i]);
  }
  if (lo < -(int64_t(1) << 45) || hi > (int64_t(1) << 45))
    return cg_fail(CG_ERANGE, "input time outside +-1.1M years");
  const int64_t kDay = 86400;
  // prev may be the zero time (no fire within five years), and Next(prev) then
  // walks from year 1; otherwise the two walks end within ~12 years of now.
  Plan plan;
  plan.table = build_table(z->rules, std::min(lo, int64_t(CG_ZERO_TIME)) - 64 * kDay,
                           hi + (12 * 366 + 64) * kDay);
  PlanArgs pa;
  int rc = upload_plan(c, plan, 0, 0, &pa);
  if (rc) return rc;
  if ((rc = c->nb_in.ensure(n)) || (rc = c->nb_out.ensure(n)) || (rc = c->lt_avg.ensure(n)) ||
      (rc = c->lt_kind.ensure(n)))
    return rc;
  HIPCHK(hipMemcpyAsync(c->nb_in.p, now, n * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->lt_kind.p, kind, n * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->lt_avg.p, avg_time_ms, n * 8, hipMemcpyHostToDevice, c->st));
  launch_lock_ttl(s->d, n, pa, c->nb_in.p, c->lt_kind.p, c->lt_avg.p, lock_ttl, c->nb_out.p, c->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ttl_out, c->nb_out.p, n * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

// -------------------------------------------------------------- utilities
int cg_checksum_device(cg_ctx* c, const void* d_ptr, int64_t n, int elem_bytes, int64_t first_index,
                       int64_t add, uint64_t* out) {
  if (!c || !out || (n > 0 && !d_ptr) || n < 0 || (elem_bytes != 8 && elem_bytes != 4))
    return cg_fail(CG_EINVAL, "cg_checksum_device: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int rc = c->cksum.ensure(1);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(c->cksum.p, 0, 8, c->st));
  launch_checksum(d_ptr, n, elem_bytes, first_index, add, c->cksum.p, c->st);
  HIPCHK(hipGetLastError());
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, c->cksum.p, 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  *out = v;
  return CG_OK;
}

int cg_fill_device(cg_ctx* c, void* d_ptr, int64_t bytes, int byte_value) {
  if (!c || bytes < 0 || (bytes > 0 && !d_ptr)) return cg_fail(CG_EINVAL, "cg_fill_device: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (bytes) HIPCHK(hipMemsetAsync(d_ptr, byte_value & 0xFF, size_t(bytes), c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

int cg_fill_rate_device(cg_ctx* c, void* d_ptr, int64_t bytes, int reps, float* ms) {
  if (!c || !ms || bytes <= 0 || bytes % 16 != 0 || !d_ptr || reps < 1)
    return cg_fail(CG_EINVAL, "cg_fill_rate_device: bad argument (bytes a positive multiple of 16, reps >= 1)");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->st));
  for (int kind = 0; kind < 3; kind++) {
    auto fill = [&]() -> hipError_t {
      if (kind == 2) return hipMemsetAsync(d_ptr, 0x5E, size_t(bytes), c->st);
      launch_fill_stream(d_ptr, bytes / 16, kind == 0, c->st);
      return hipGetLastError();
    };
    HIPCHK(fill());  // warm-up
    HIPCHK(hipEventRecord(c->ev[0], c->st));
    for (int r = 0; r < reps; r++) HIPCHK(fill());
    HIPCHK(hipEventRecord(c->ev[1], c->st));
    HIPCHK(hipEventSynchronize(c->ev[1]));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
    ms[kind] = t / float(reps);
  }
  return CG_OK;
}

int cg_count_value_device(cg_ctx* c, const void* d_ptr, int64_t n, int elem_bytes, int64_t value,
                          int64_t* count) {
  if (!c || !count || (n > 0 && !d_ptr) || n < 0 || (elem_bytes != 8 && elem_bytes != 4))
    return cg_fail(CG_EINVAL, "cg_count_value_device: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int rc = c->cksum.ensure(1);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(c->cksum.p, 0, 8, c->st));
  launch_count_eq(d_ptr, n, elem_bytes, value, c->cksum.p, c->st);
  HIPCHK(hipGetLastError());
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, c->cksum.p, 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  *count = int64_t(v);
  return CG_OK;
}

int cg_set_phase_timing(cg_ctx* c, int level) {
  if (!c || level < 1 || level > 2) return cg_fail(CG_EINVAL, "cg_set_phase_timing: level 1 or 2");
  std::lock_guard<std::mutex> g(c->mu);
  c->phase_timing = level;
  return CG_OK;
}

int cg_set_node_order(cg_ctx* c, int order) {
  if (!c || (order != CG_NODE_ORDER_RULE && order != CG_NODE_ORDER_TIME))
    return cg_fail(CG_EINVAL, "cg_set_node_order: CG_NODE_ORDER_RULE or CG_NODE_ORDER_TIME");
  std::lock_guard<std::mutex> g(c->mu);
  c->node_order = order;
  return CG_OK;
}

int cg_last_kernel_times(cg_ctx* c, float* ms, int n) {
  if (!c || !ms) return cg_fail(CG_EINVAL, "cg_last_kernel_times: null");
  int k = std::min(n, int(KT_COUNT));
  for (int i = 0; i < k; i++) ms[i] = c->kt[i];
  return k;
}

}  // extern "C"
