// cg_api_internal.h -- context/specs objects behind the C-ABI handles, and the
// state the expansion paths share: RunSet (a rule-major count/scan/write chain
// with its plan; one for the synchronous path, one per pipelined set) and
// PnWindow (a per-node window's chain), each owned once by cg_ctx and once by
// every set of the matching pipeline (AsyncSet, PnAsyncSet).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_kernels.h"
#include "cg_zone.h"

int cg_fail(int code, const std::string& msg);
int cg_hip_check(hipError_t e, const char* what);

#define HIPCHK(x)                    \
  do {                               \
    int _rc = cg_hip_check((x), #x); \
    if (_rc != CG_OK) return _rc;    \
  } while (0)

// per rule of a per-node window (k_rule_info): fire count, band-relative
// index of the first fire, and {first - t0, stride} of a progression (st 0:
// not one)
struct alignas(16) RuleInfo {
  int32_t cnt, off, first, st;
};

// per-node writer record of one non-empty (node, rule) pair of a segment
// (cg_pernode.hip, k_seg_records): rule, first position in the segment, and
// x, st -- fire at position p = t0 + x + p * st (a progression rule), or
// band-relative fire-list index = x + p when st == 0
struct alignas(16) PairRec {
  int32_t rule, dst, x, st;
};

// blocks of `threads` items for n items: at least one, at most cap
inline int gridn(int64_t n, int threads, int cap) {
  int64_t b = (n + threads - 1) / threads;
  if (b < 1) b = 1;
  return int(std::min<int64_t>(b, cap));
}

// Grow-only device buffer (grows by 1.25x so repeated calls settle).
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return CG_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    size_t want = std::max(n, cap + cap / 4);
    hipError_t e = hipMalloc(&p, want * sizeof(T));
    if (e != hipSuccess) {
      // retry at the exact size before giving up
      e = hipMalloc(&p, n * sizeof(T));
      if (e != hipSuccess) {
        p = nullptr;
        cap = 0;
        return cg_hip_check(e, "hipMalloc");
      }
      want = n;
    }
    cap = want;
    return CG_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// An integer-interned rule set in device memory (cg_rules_in uploaded).
struct RulesStore {
  DBuf<int64_t> nid_off, gid_off, ex_off, group_off;
  DBuf<int32_t> nids, gids, ex, group_nodes, rule_job;
  // next_same[r]: the next rule of r's job with r's Cmd key (rule_key), or -1
  // (Job.Cmds keeps the last included rule per key, job.go:604-609); only
  // uploaded when some job repeats a key (has_dup); prev_same[r] the previous
  // one (k_rule_nodes sweeps each key's chain from its last rule back)
  DBuf<int32_t> next_same, prev_same;
  bool has_dup = false;
  DBuf<uint8_t> group_exists, job_pause;
  int32_t n_nodes = 0, n_groups = 0, n_rules = 0, n_jobs = 0;
  uint64_t serial = 0;  // unique per upload: keys the per-node transpose cache
  void release() {
    nid_off.release(); gid_off.release(); ex_off.release(); group_off.release();
    nids.release(); gids.release(); ex.release(); group_nodes.release(); rule_job.release();
    next_same.release(); prev_same.release();
    group_exists.release(); job_pause.release();
  }
};

// One run set of the rule-major expansion (cg_expand.cpp): what the count and
// scan of a call write and its writer reads, with the call's plan.  The
// synchronous path has one (cg_ctx::rs), every pipelined set its own, so the
// count and scan of call k (on the ctx's second stream) can run while the
// writer of call k-1 reads another.
struct RunSet {
  DBuf<int64_t> run_anchor, run_off, offsets, block_run;
  DBuf<int32_t> run_count;
  DBuf<uint32_t> run_dmask;
  DBuf<char> scan_tmp, plan_dev;
  DBuf<unsigned long long> stuck;
  // {E, stuck rule}: mapped, coherent pinned memory the scan kernel stores
  // straight into (no D2H copy launch); read once the scan's stream has drained
  int64_t* res_host = nullptr;
  int64_t* res_dev = nullptr;
  char* plan_pin = nullptr;  // pinned staging of the plan upload
  size_t plan_pin_cap = 0;
  // the plan in plan_dev, kept across calls with the same (zone, t0, t1)
  cg::Plan plan;
  cg::PlanArgs pa{};
  bool plan_valid = false;
  uint64_t plan_zone = 0;
  int64_t plan_t0 = 0, plan_t1 = 0;
  // the plan's zone table reaches as far as cg_lock_ttl_batch's (a lock
  // profile's; lock_table of run_set_count_scan): part of the cache key
  bool plan_lock_table = false;
  // The stuck word holds ~0 whenever a count starts: k_count only lowers it
  // (atomicMin of a stuck rule) and the scan behind it copies it into the
  // record and stores ~0 again.  run_set_count_scan sets it once, before the
  // set's first count, and from then on never returns between enqueueing a
  // count and its scan (every allocation comes first), so every count that was
  // enqueued has a scan behind it that re-arms the word.
  bool armed = false;
  int64_t R = 0, cap = 0;  // rules and slice-map capacity of the last count and scan
  // walked runs: WALK windows, or CF segments whose entry fire does not fully
  // match (only possible when the plan has zone transitions; a CF run is
  // entered by the exact walk only after a WALK segment, or from T0 when a
  // transition lies in the 40 days before it)
  bool has_walk() const { return (plan.flags & (cg::kPlanT0Walk | cg::kPlanWalkSegs)) != 0; }
  int ensure_res() {
    if (res_host) return CG_OK;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&res_host), 16, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&res_dev), res_host, 0));
    res_host[0] = 0;
    res_host[1] = -1;
    return CG_OK;
  }
  void release() {
    run_anchor.release(); run_off.release(); offsets.release(); block_run.release();
    run_count.release(); run_dmask.release(); scan_tmp.release(); plan_dev.release(); stuck.release();
    if (res_host) (void)hipHostFree(res_host);
    if (plan_pin) (void)hipHostFree(plan_pin);
    res_host = res_dev = nullptr;
    plan_pin = nullptr;
    plan_pin_cap = 0;
  }
};

// One set of the pipelined expansion (cg_expand_device_async): a run set and
// the bookkeeping of the call that last used it.
struct AsyncSet {
  RunSet rs;
  hipEvent_t written = nullptr;  // recorded behind the walk writer
  // the set's writer-done event of its last call: `written`, or without a walk
  // kernel the call's end-of-writer timing event (not owned; null: none yet)
  hipEvent_t done = nullptr;
  int tslot = 0;   // the call's pair in the ctx's timing-event ring
  int tprev = -1;  // the previous call's pair when its writer may overlap this one's (-1: none)
  bool pending = false;  // a call on this set whose record has not been checked
  void release() {
    rs.release();
    if (written) (void)hipEventDestroy(written), written = nullptr;
    done = nullptr;
  }
};

// One per-node window's device chain (cg_pernode.hip): what pn_records_enqueue
// builds from the window's rule-major fire lists and pn_writer_enqueue reads.
// The synchronous path has one (cg_ctx::pn), every pipelined set its own.
struct PnWindow {
  DBuf<RuleInfo> rule_info;         // per rule (k_rule_info)
  DBuf<int64_t> seg_cnt, seg_pos;   // per (node, band) segment: events, their scan [N*K+1]
  DBuf<int32_t> seg_nrec;           // per segment: non-empty pairs
  DBuf<PairRec> recs;               // their records (k_seg_records)
  DBuf<uint32_t> tickets;           // the writer's task tickets
  // the owner's node offsets [N+1] and scan temporary (not owned: the
  // synchronous path's are the ctx's readable result and shared temporary)
  int64_t* node_off = nullptr;
  void* scan_tmp = nullptr;
  // mapped pinned result words: [0] node events, [1] size error, [2] order check
  int64_t* res_host = nullptr;
  int64_t* res_dev = nullptr;
  // the window pn_records_enqueue was last given (the writer's arguments)
  const int64_t* offsets = nullptr;
  const int64_t* times = nullptr;
  int64_t t0 = 0;
  int32_t N = 0, K = 0, B = 0;
  int ensure_res() {
    if (res_host) return CG_OK;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&res_host), 32, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&res_dev), res_host, 0));
    res_host[0] = res_host[1] = res_host[2] = 0;
    return CG_OK;
  }
  void release() {
    rule_info.release(); seg_cnt.release(); seg_pos.release(); seg_nrec.release();
    recs.release(); tickets.release();
    if (res_host) (void)hipHostFree(res_host);
    res_host = res_dev = nullptr;
  }
};

// One set of the pipelined per-node path (cg_expand_per_node_rules_device_async):
// the window's rule-major expansion (its own run set and fire times) and its
// chain, so window k+1's expansion and records are built on the second stream
// while window k's per-node writer streams on the first.
struct PnAsyncSet {
  RunSet rm;
  PnWindow w;
  DBuf<int64_t> times, node_off;
  DBuf<char> seg_tmp;
  hipEvent_t side_done = nullptr, written = nullptr, nw0 = nullptr, nw1 = nullptr;
  bool pending = false;
  bool timed = false;  // the window's lists are written in (time, rule) order
  int64_t t0 = 0, t1 = 0, node_cap = 0, rm_cap = 0;
  int32_t N = 0;
  void release() {
    rm.release();
    w.release();
    times.release(); node_off.release(); seg_tmp.release();
    for (hipEvent_t* e : {&side_done, &written, &nw0, &nw1})
      if (*e) (void)hipEventDestroy(*e), *e = nullptr;
  }
};

// Slots of cg_ctx::kt, the milliseconds cg_last_kernel_times reports.  The
// values are public: engine.py and the tools read the slots by number.
enum Kt {
  KT_X_COUNT = 0,        // expansion: k_count
  KT_X_SCAN = 1,         // scan of the run counts
  KT_X_MAP = 2,          // slice map
  KT_X_WRITE_CF = 3,     // k_write_cf (pipelined calls: the mean of the calls checked)
  KT_X_WRITE_WALK = 4,   // k_write_walk
  KT_X_OFFSETS = 5,      // per-rule offsets (0: written by the scan)
  KT_PN_JOIN = 6,        // last per-node call: rule->node join
  KT_PN_TRANSPOSE = 7,   // transpose + per-node offsets
  KT_PN_WRITE = 8,       // k_node_write (pipelined windows: the mean of the calls checked)
  KT_DISP_SCAN = 9,      // last cg_dispatcher_fire: scan
  KT_DISP_DUE = 10,      // due compaction
  KT_DISP_ADVANCE = 11,  // advance
  KT_TIME_ORDER = 12,    // time-order pass of the last cg_node_result_order_by_time
  KT_FANOUT = 13,        // last cg_dispatcher_fanout
  KT_PF_RULES = 14,      // last profile call: k_profile_rules / k_inflight_rules
  KT_PF_WALK = 15,       // k_profile_walk / k_inflight_walk (a unit call: up to k_admit_prepare)
  KT_PF_TOTALS = 16,     // k_profile_totals
  KT_PF_JOIN = 17,       // join + transpose (0: the cached one was reused)
  KT_PF_NODES = 18,      // node matrix
  KT_UNIT_PREPARE = 19,  // k_admit_prepare of an admission or lock call (0 after any other)
  KT_ADMIT_UNITS = 20,   // k_admit_units
  KT_LOCK_UNITS = 21,    // k_lock_units
  KT_ROWS_PREFIX = 22,   // k_rows_prefix of a RUNNING call
  KT_COUNT
};
static_assert(KT_COUNT == 23, "cg_last_kernel_times' slots are public");
// cg_ctx::pfev: where a profile call records each event on the ctx stream
enum PfEv {
  PFEV_RULES = 0,      // before the rule-matrix kernel
  PFEV_WALK = 1,       // before the walked runs' kernel
  PFEV_TOTALS = 2,     // before k_profile_totals: the end of the unit walk, in a RUNNING call of k_rows_prefix
  PFEV_TOTALS_END = 3, // where a per-node call's join starts
  PFEV_NODES = 4,      // before the node matrix
  PFEV_NODES_END = 5,
  PFEV_PREPARE = 6,    // before k_admit_prepare
  PFEV_UNITS = 7,      // before the unit walk
  PFEV_PREFIX = 8,     // RUNNING calls: the end of the unit walk, before k_rows_prefix
  PFEV_COUNT
};
// cg_ctx::vdev: a verdict call's events, then a selection's
enum VdEv {
  VDEV_EXPAND = 0,     // before the plain expansion
  VDEV_INIT = 1,       // before k_verdict_init (behind the uploads)
  VDEV_ADMIT = 2,      // before k_admit_verdicts
  VDEV_LOCK = 3,       // before k_lock_verdicts
  VDEV_WALKS_END = 4,
  VDEV_SEL_COUNT = 5,  // before k_verdict_count
  VDEV_SELECT = 6,     // after the count's scan; recorded again before k_verdict_select
  VDEV_SELECT_END = 7,
  VDEV_COUNT
};

// the timing events of one entry-point family, created on first use
template <size_t N>
int ensure_events(hipEvent_t (&evs)[N]) {
  for (hipEvent_t& e : evs)
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  return CG_OK;
}

struct cg_ctx {
  int device = 0;
  int write_blocks = 1024;  // persistent k_write_cf grid (set from the CU count)
  int write_blocks_ov = 1024;  // of each of two overlapped pipelined writers (kWriteBlocksPerCUOverlap)
  hipStream_t st = nullptr;
  hipEvent_t ev[8] = {};
  hipEvent_t pev[4] = {};  // per-node phases
  std::mutex mu;
  float kt[KT_COUNT] = {};  // cg_last_kernel_times: ms per slot (enum Kt)
  // expansion phase timing: 2 = an event between every phase (KT_X_COUNT..KT_X_OFFSETS);
  // 1 = events around k_write_cf only (KT_X_WRITE_CF; the others read -1).  Each
  // event recorded between two kernels costs 6-12 us of idle GPU on this
  // stack, so throughput runs use 1 (cg_set_phase_timing).
  int phase_timing = 2;

  // the zone table of a Next / lockTtl batch (upload_plan)
  std::vector<char> plan_host;
  DBuf<char> plan_dev;

  // synchronous expansion: its run set and the output (the pipelined path's
  // first output buffer too); Next / lockTtl batches; the shared temporary of
  // the join, transpose, segment and time-order scans
  RunSet rs;
  DBuf<int64_t> times, nb_in, nb_out, lt_avg;
  DBuf<int32_t> lt_kind;
  DBuf<char> scan_tmp;
  DBuf<unsigned long long> cksum;  // cg_checksum_device accumulator
  int64_t last_E = 0, last_R = 0;
  // counts the calls that replace (or clear) the readable rule-major result:
  // every synchronous count chain, pipelined call and pipelined per-node window
  uint64_t res_gen = 0;

  // fire verdicts (cg_verdict.hip): one byte per fire of the rule-major result
  // of generation vd_gen (vd_R rules, vd_E fires), and the last selection
  // (sel_off [vd_R + 1], sel_times [vd_nsel])
  DBuf<uint8_t> vd_verdict;
  DBuf<int32_t> vd_sel_cnt;
  DBuf<int64_t> vd_sel_off, vd_sel_times;
  uint64_t vd_gen = 0;
  int64_t vd_R = 0, vd_E = 0, vd_nsel = 0;
  bool vd_valid = false, vd_sel_valid = false;
  float vd_ms[6] = {0, 0, 0, 0, 0, 0};  // cg_verdict_times
  hipEvent_t vdev[VDEV_COUNT] = {};

  // pipelined expansion (cg_async.cpp): the sets used in turn, count + scan
  // on st_cs, writers on st / st_w1; as_last = set of the last async result
  // (-1: the last result came from the synchronous path)
  // Three run sets: a call's count and scan are enqueued while the writer
  // two calls back is long done, so they sit ready in the hardware queue and
  // run in the previous writer's tail instead of racing the next writer's
  // start (two sets: the count alternately ran before and after that start,
  // 19 vs 50 us between writers, profiles/r02_ab_async_sets.json)
#ifndef CG_ASYNC_SETS
#define CG_ASYNC_SETS 3
#endif
  static constexpr int kAsyncSets = CG_ASYNC_SETS;
  AsyncSet as[kAsyncSets];
  int as_next = 0, as_last = -1;
  hipStream_t st_cs = nullptr;
  hipEvent_t cs_done[kAsyncSets] = {};
  int async_rc = 0;  // first error of the calls since the last cg_expand_wait
  std::string async_msg;
  double wr_ms_sum = 0;  // writer (k_write_cf) time of the checked async calls
  int wr_n = 0;
  // Writer overlap: pipelined call k runs its writer on writer stream k & 1
  // (st, st_w1) into output buffer k & 1 (times, times2), so two writers are
  // resident side by side and the stores never pause between calls
  // (pipelined steps).  Writers k and k+2
  // share a stream and a buffer (stream order); neighbours share nothing they
  // write.  times2 holds at least times.cap events while the overlap is
  // active; without it every call uses st and times.
  hipStream_t st_w1 = nullptr;
  DBuf<int64_t> times2;
  bool ov_on = true;       // cg_set_async_overlap
  bool ov_active = false;  // decided by a pipelined call made with nothing pending
  bool w1_dirty = false;   // work enqueued on st_w1 since it was last synchronised
  unsigned wr_call = 0;    // pipelined calls so far: its parity picks stream and buffer
  int times_last = 0;      // the output buffer of the last result (0: times, 1: times2)
  // writer start / end events of the pipelined calls: a ring one deeper than
  // the run sets, so the previous call's end is still there when a call is
  // checked (cg_async.cpp, check_set)
  static constexpr int kTimeRing = kAsyncSets + 1;
  hipEvent_t tw0[kTimeRing] = {}, tw1[kTimeRing] = {};
  int tw_next = 0, tw_prev = -1;  // next pair; the previous call's since the last drain (-1: none)
  int64_t* result_times() const { return times_last ? times2.p : times.p; }

  // pipelined per-node windows (cg_pernode.hip): three sets in turn
  static constexpr int kPnSets = 3;
  PnAsyncSet pns[kPnSets];
  int pa_next = 0, pa_last = -1;
  int pa_rc = 0;  // first error of the per-node calls since the last wait
  std::string pa_msg;
  double nw_ms_sum = 0;  // per-node writer time of the checked calls
  int nw_n = 0;
  int64_t pa_en_sum = 0;  // node events of the checked calls since the last wait

  // per-node buffers: the rule->node join (rule-major pairs), its node-major
  // transpose, the (node, rule band) segment bounds, the node CSR and the
  // synchronous path's window chain
  DBuf<int64_t> rn_off, node_off, node_time, nt_off, rs_off, seg_pair;
  DBuf<int32_t> rn_cnt, rn_nodes, pair_node, pair_rule, node_rule, nt_rule, rs_hist;
  PnWindow pn;
  // time-order pass (cg_node_order.hip): node-aligned tiles, per-pass
  // histograms/offsets, and the second buffers of the ping-pong
  DBuf<int32_t> ts_cnt, ts_tile_node, ts_hist, node_rule2;
  DBuf<int64_t> ts_base, ts_off, node_time2, ts_node_off;
  DBuf<int64_t> ts_start;  // per tile its first list position; [T] = the lists' end
  DBuf<int32_t> ts_hi;     // per tile the high rule bits (rule >> 20) all its events share
  int64_t pn_t0 = 0, pn_t1 = 0;  // window of the last per-node result
  RulesStore rules;  // rule set of the host-array entry points (re-uploaded per call)
  int64_t pn_E = 0, pn_nnz = 0, pn_N = 0;
  // a per-node result is readable (node_off [pn_N+1], pn_E events): cleared
  // when a per-node call starts or fails, set when one succeeds -- pn_N and
  // node_off may be stale otherwise (the gather / node offsets check it)
  bool pn_valid = false;
  int64_t pn_R = INT64_MAX;  // rule count of the per-node lists being ordered (the merge packs rules below 2^20)
  // time-ordered gather (merge_ranks_enqueue): per-node run bounds, the tile
  // prefix over runs, and a scratch copy of one node group
  DBuf<int64_t> mr_rb, mr_tp, mr_t;
  DBuf<int32_t> mr_r;
  // the rule->node join + transpose depend only on (rule set, exclude mode):
  // kept across per-node calls on the same uploaded rule set (time windows);
  // the segment bounds also on the band width
  uint64_t pn_cache_serial = 0;
  int pn_cache_mode = -1;
  int node_order = CG_NODE_ORDER_RULE;  // cg_set_node_order
  bool pn_time_ordered = false;         // the last per-node result is in (time, rule) order
  int32_t pn_B = 0, pn_K = 0;  // rules per band, bands of the cached segment bounds (0: none)
  // the time-order merge's dense nodes run on their own stream beside the
  // sparse ones (fork / join events on st)
  hipStream_t st_ot = nullptr;
  hipEvent_t ot_fork = nullptr, ot_join = nullptr;

  // fire profile (cg_profile.hip): the matrices of the last profile call --
  // rule counts [pf_R][pf_B], bucket totals [pf_B], node counts [pf_N][pf_B]
  // (pf_has_nodes) -- in buffers no other entry point touches; the chunk
  // counts / offsets of the nodes' rule lists and the heavy nodes' partials
  DBuf<int32_t> pf_rules, pf_chunk_cnt;
  DBuf<int64_t> pf_totals, pf_nodes, pf_part, pf_chunk_off;
  int64_t pf_R = 0;
  int32_t pf_N = 0, pf_B = 0;
  bool pf_valid = false, pf_has_nodes = false;
  // starts or in flight (CG_PROFILE_*); an in-flight call's durations in
  // whole seconds [R], uploaded per call; the node matrix's row peaks
  // (cg_profile_node_peaks: computed on first use after a profile call)
  int pf_kind = CG_PROFILE_STARTS;
  DBuf<int64_t> pf_dur, pf_peak;
  DBuf<int32_t> pf_peak_bucket;
  bool pf_peaks_valid = false;
  // The per-call uploads of a unit walk (cg_units.h, unit_upload), shared by
  // the profile and the verdict calls: every user holds mu for the whole call
  // and nothing reads them once it has ended.  Slot 0 admission, slot 1 lock
  // (a verdict call walks both): the compacted units (cg::AdmitUnit 24 B,
  // cg::LockUnit 32 B each), per-rule flags [R] ([0] "unit can drop", of a
  // verdict call the initial verdict bytes; [1] "contending rule of a lock
  // unit") and two error words the kernels lower from ~0 ([0] verdict position
  // mismatch, [1] the lock walk's rule whose Next never returns)
  DBuf<char> uw_units[2];
  DBuf<uint8_t> uw_flag[2];
  DBuf<unsigned long long> uw_err;
  hipEvent_t pfev[PFEV_COUNT] = {};  // created by the first profile call
  // The node matrix is summed over nt_off / nt_rule, which are the per-node
  // path's cache and may be rebuilt under a readable profile: nt_gen counts
  // the rebuilds (transpose_locked, and the dispatcher bind that takes the
  // buffers), pf_nt_gen / pf_nnz are the transpose of the last per-node profile
  uint64_t nt_gen = 0, pf_nt_gen = 0;
  int64_t pf_nnz = 0;
  // top rules of a bucket (cg_top_rules.hip): the last result -- tr_rows rows
  // of tr_k (rule, count) columns plus three words per row -- and the split
  // rows' per-chunk lists (keys, non-zero counts) in buffers of their own
  DBuf<int32_t> tr_rule, tr_cnt, tr_nlisted, tr_ncontrib, tr_bucket, tr_part_nz;
  DBuf<unsigned long long> tr_part;
  int32_t tr_rows = 0, tr_k = 0;
  bool tr_valid = false;
  float tr_ms[3] = {0, 0, 0};  // select, merge, chunks (cg_profile_top_rules_times)
  hipEvent_t trev[3] = {};

  void free_all() {
    tr_rule.release(); tr_cnt.release(); tr_nlisted.release(); tr_ncontrib.release();
    tr_bucket.release(); tr_part_nz.release(); tr_part.release();
    for (hipEvent_t& e : trev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    for (AsyncSet& a : as) a.release();
    for (PnAsyncSet& a : pns) a.release();
    for (hipEvent_t& e : cs_done)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    for (hipEvent_t* ring : {tw0, tw1})
      for (int i = 0; i < kTimeRing; i++)
        if (ring[i]) (void)hipEventDestroy(ring[i]), ring[i] = nullptr;
    if (st_cs) (void)hipStreamDestroy(st_cs);
    st_cs = nullptr;
    if (st_w1) (void)hipStreamDestroy(st_w1);
    st_w1 = nullptr;
    times2.release();
    if (ot_fork) (void)hipEventDestroy(ot_fork), ot_fork = nullptr;
    if (ot_join) (void)hipEventDestroy(ot_join), ot_join = nullptr;
    if (st_ot) (void)hipStreamDestroy(st_ot);
    st_ot = nullptr;
    plan_dev.release();
    rs.release(); times.release();
    nb_in.release(); nb_out.release(); lt_avg.release(); lt_kind.release();
    scan_tmp.release(); cksum.release();
    rn_off.release(); node_off.release(); node_time.release(); nt_off.release(); rs_off.release();
    seg_pair.release(); rn_cnt.release(); rn_nodes.release();
    pair_node.release(); pair_rule.release(); node_rule.release(); nt_rule.release();
    rs_hist.release(); pn.release(); rules.release();
    ts_cnt.release(); ts_tile_node.release(); ts_hist.release(); node_rule2.release();
    ts_start.release(); ts_hi.release();
    ts_base.release(); ts_off.release(); node_time2.release(); ts_node_off.release();
    mr_rb.release(); mr_tp.release(); mr_t.release(); mr_r.release();
    pf_rules.release(); pf_chunk_cnt.release(); pf_totals.release(); pf_nodes.release();
    pf_part.release(); pf_chunk_off.release();
    pf_dur.release(); pf_peak.release(); pf_peak_bucket.release();
    for (int i = 0; i < 2; i++) uw_units[i].release(), uw_flag[i].release();
    uw_err.release();
    for (hipEvent_t& e : pfev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    vd_verdict.release(); vd_sel_cnt.release(); vd_sel_off.release(); vd_sel_times.release();
    for (hipEvent_t& e : vdev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
  }
};

struct cg_rules {
  cg_ctx* ctx = nullptr;
  RulesStore st;
};

struct cg_zone {
  cg::ZoneRules rules;
  uint64_t serial;
};

struct cg_specs {
  cg_ctx* ctx = nullptr;
  cg::DSpec* d = nullptr;
  size_t n = 0;
  bool owner = false;
};

// cg_schedule -> packed 32-byte device spec (validates @every delays)
int pack_spec(const cg_schedule& s, cg::DSpec* d);
int upload_plan(cg_ctx* c, const cg::Plan& plan, int64_t t0, int64_t t1, cg::PlanArgs* pa);
struct PlanLayout {
  size_t o_when, o_off, o_seg, o_dt, bytes;
};
PlanLayout plan_layout(const cg::Plan& plan);
void plan_pack(const cg::Plan& plan, const PlanLayout& L, char* dst);
int plan_args(const cg::Plan& plan, const PlanLayout& L, char* dev_base, int64_t t0, int64_t t1,
              cg::PlanArgs* pa);
// The rule-major chain every expansion entry point runs (cg_expand.cpp).
// run_set_count_scan stages the plan of (t0, t1] in zone z into rs (cached per
// (zone, t0, t1); through the set's pinned buffer, no stream sync) and
// enqueues k_count and the scan of the run counts on st: rs.run_off then holds
// the run offsets, rs.offsets the rule offsets and the set's record {E, stuck
// rule}.  map_cap > 0: the scan also builds k_write_cf's slice map for an
// output capacity of map_cap events (no k_chunk_map launch).  ev (or null):
// three events recorded before the count, between the two and after the scan.
// lock_table: the staged zone table reaches from the zero time to 12 years past
// t1 (a lock profile's Next calls); segments, windows and flags are unchanged.
// *empty: no rule or no segment -- nothing is counted, the record reads {0,
// none} and rs.offsets [R+1] is left for the caller to zero.  The caller has
// made sure that nothing enqueued earlier still reads or writes rs.
int run_set_count_scan(RunSet& rs, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1, int64_t map_cap,
                       hipStream_t st, hipEvent_t* ev, bool* empty, bool lock_table = false);
// What a synchronous call does before its count and scan on the ctx stream
// into c->rs (cg_expand.cpp): drains and discards pending pipelined calls,
// clears the readable rule-major result, checks the horizon; an empty call's
// offsets are zeroed and the stream drained.  c->mu held.
int sync_count_scan(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1, bool* empty,
                    int64_t map_cap = 0, bool lock_table = false);
// the writers of the runs counted last into out (cap events: the capacity the
// slice map was built for), on st: k_write_cf on `blocks` blocks, after_cf (or
// null) recorded behind it, then k_write_walk when the plan has walked runs
void run_set_write_enqueue(const RunSet& rs, const cg_specs* s, int64_t cap, int64_t* out, int blocks,
                           hipStream_t st, hipEvent_t after_cf = nullptr);
// the error text of a record whose stuck rule is not ~0
std::string stuck_msg(unsigned long long rule);
// (lock_table: the count chain stages the lock profile's zone table, for the
// walk a verdict call runs behind the writers; the result is the same)
int expand_device_locked(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                         int64_t* n_events, bool lock_table = false);
// finish and check every pending cg_expand_device_async call (cg_async.cpp);
// their errors are reported by the next cg_expand_wait
int async_drain(cg_ctx* c);
int ensure_async(cg_ctx* c);  // the second stream and the pipelined sets' events
bool async_pending(const cg_ctx* c);
// pipelined per-node calls (cg_pernode.hip): drain (errors kept for the next
// wait) / any pending
int pn_async_drain(cg_ctx* c);
bool pn_async_pending(const cg_ctx* c);  // an asynchronous expansion not yet waited for
// the rule->node join of a rule set under an exclude mode, left in the ctx's
// shared join buffers (rn_off [R+1], rn_nodes / pair_rule [nnz]), and its
// stable node-major transpose (nt_off [N+1], nt_rule [nnz]; rn_nodes /
// pair_rule are consumed); c->mu held.  The per-node path caches these buffers
// by (pn_cache_serial, pn_cache_mode): any other caller clears pn_cache_serial.
// (cg_rule_nodes.hip; upload_rules validates a host rule set and copies it into a device store)
int upload_rules(const cg_rules_in* in, RulesStore* st, hipStream_t s);
int rule_nodes_locked(cg_ctx* c, const RulesStore& st, int mode, int64_t* nnz_out);
int transpose_locked(cg_ctx* c, int64_t nnz, int32_t N);
// rules of a node's list per chunk of the node-matrix sum and of the top-rules
// select (pf_chunk_off: the exclusive scan of the nodes' chunk counts; a node
// without rules still has one chunk)
constexpr int kNodeChunk = 512;
// k_node_peaks over the readable profile's node matrix (pf_N > 0 rows) into
// pf_peak / pf_peak_bucket [pf_N], which the caller has sized, on the ctx
// stream; the caller sets pf_peaks_valid once the stream has drained
int profile_node_peaks_enqueue(cg_ctx* c);
// The transpose's stable LSD passes (k_rs_hist / k_rs_scatter, 8 bits a pass)
// over n (key, value) pairs with keys < N, ping-ponging between (k0, v0) and
// (k1, v1); *in_second: the sorted pairs are in (k1, v1).  hist needs
// radix_hist_words(n) int32, off one more int64, scan_tmp scan_temp_bytes of
// that count.  Enqueued on st.
int64_t radix_hist_words(int64_t n);
void radix_by_key_enqueue(hipStream_t st, uint32_t* k0, int32_t* v0, uint32_t* k1, int32_t* v1, int64_t n,
                          int32_t N, int32_t* hist, int64_t* off, void* scan_tmp, bool* in_second);
// off[v] = first index of the sorted keys with keys[i] >= v, v in [0, N] (k_node_bounds)
void launch_node_bounds(hipStream_t st, const uint32_t* keys, int64_t n, int32_t N, int64_t* off);
// time-order tile sort + merge of c->node_time / c->node_rule (windows <= 4096 s;
// cg_node_order.hip), enqueued on st without a host sync
// in_mode: what the writer left in c->node_time / c->node_rule -- kInTimes
// int64 times + rules; kIn16 16-bit offsets t - t0 - 1 + rules
// (k_node_write<.., kIn16>); kInPacked one word per event, offset << 20 |
// (rule & 0xFFFFF), in c->node_rule (k_node_write<.., kInPacked>; rules <
// 2^24: past 2^20 the tiles are cut where rule >> 20 changes and carry it)
constexpr int kInTimes = 0, kIn16 = 1, kInPacked = 2;
// the time-order writer may emit kInPacked for R rules (indices < 2^24)
bool pn_pack_ok(int64_t R);
// where every node's list crosses a multiple of 2^20 in rule index: the
// (node, band) segment offsets seg_pos [N*K+1] of bands of B rules (B a power
// of two <= 2^20, so 2^20 / B bands per block of 2^20 rules); null seg_pos:
// no cuts (rule indices < 2^20)
struct TileCut {
  const int64_t* seg_pos = nullptr;
  int32_t K = 1, B = 1;
  int64_t R = 0;
};
// err: a device word the kernels set when a sorted chunk is out of (time,
// rule) order (the sorts' ranks rest on lane-ordered LDS atomics; checked)
int order_merge_enqueue(cg_ctx* c, const int64_t* node_off, int32_t N, int64_t cap, int64_t t0, int64_t H,
                        hipStream_t st, int in_mode, int64_t* err, const TileCut& cut = TileCut());
constexpr const char* kOrderCheckMsg =
    "time-order pass: a sorted chunk came out of (time, rule) order (its LDS-atomic ranks were not in lane order)";
// the time-order pass over the last (rule-major) per-node result; c->mu held
int order_by_time_locked(cg_ctx* c, int in_mode = 0);
// kernels of the per-node CSR gather (cg_node_gather.hip), enqueued on st:
// node n's events [src_off[n], src_off[n+1]) of src to dst_start[n] onwards /
// n contiguous events / the last per-node result's counts per node
// (event i of src_off's numbering at src_*[i - src_shift])
int launch_node_place(cg_ctx* c, hipStream_t st, int32_t N, const int64_t* src_off, int64_t src_shift,
                      const int64_t* src_time, const int32_t* src_rule, int32_t rule_add, const int64_t* dst_start,
                      int64_t* dst_time, int32_t* dst_rule);
int launch_span_place(cg_ctx* c, hipStream_t st, int64_t n, const int64_t* src_time, const int32_t* src_rule,
                      int32_t rule_add, int64_t* dst_time, int32_t* dst_rule);
int launch_node_counts(cg_ctx* c, hipStream_t st, int64_t* d_counts);
// Time-ordered gather: every node's list in d_time / d_rule holds W runs (the
// ranks' slices in rank = job-ID order, each in (time, rule) order); h_rb
// [N*(W+1)] (host) are the run bounds, node-major: run g of node n is
// [h_rb[n*(W+1)+g], h_rb[n*(W+1)+g+1]).  Merges every node's runs in place
// into (time, rule) order, one group of nodes of at most scratch_ev events at
// a time (a larger node alone) through a scratch copy (scr_t / scr_r), on st;
// returns after the stream has drained.
int merge_ranks_locked(cg_ctx* c, hipStream_t st, int32_t N, int32_t W, const int64_t* h_rb, int64_t* d_time,
                       int32_t* d_rule, int64_t scratch_ev, DBuf<int64_t>& scr_t, DBuf<int32_t>& scr_r);
constexpr int kMergeMaxRanks = 64;
// CG_ORDER_LSD set: order every window by the LSD passes (int64 times; the
// writer must not emit 16-bit offsets then)
bool order_lsd_only();
