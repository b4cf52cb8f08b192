// cg_dispatcher.h -- the object behind a cg_dispatcher handle (cg_dispatch.cpp
// owns the wake; cg_fanout.hip the node fan-out of a wake).
#pragma once
#include <vector>

#include "cg_api_internal.h"

// Node fan-out of a wake (cg_fanout.hip): the bound rule set's join and the
// last result, all owned by the dispatcher.
struct DispatchFanout {
  bool bound = false;
  int32_t N = 0;      // nodes of the bound rule set
  int64_t R = 0;      // its rules: slot i < R is rule i
  int64_t nnz = 0;    // (rule, node) pairs of the join
  int path = CG_FANOUT_AUTO;
  int mode = 0;       // the exclude mode it was bound with (patches join under it)
  // rule -> nodes CSR and its stable node-major transpose (rules ascending
  // within a node)
  DBuf<int64_t> rn_off, nt_off;
  DBuf<int32_t> rn_nodes, nt_rule;
  // result: node_off [N+1], slots [n_pairs]
  DBuf<int64_t> node_off;
  DBuf<int32_t> slots;
  int64_t n_pairs = 0;
  bool valid = false;  // a result of the last wake is readable
  // filter path: due pairs per tile of the transpose, their scan
  DBuf<int32_t> tile_cnt;
  DBuf<int64_t> tile_base;
  // due-driven path: degrees of the due slots, their scan, the (node, slot)
  // pairs in due order and the ping-pong of the sort
  DBuf<int32_t> deg, key0, key1, val1, hist;
  DBuf<int64_t> deg_off, hist_off;
  DBuf<char> scan_tmp;
  // cg_dispatcher_patch_rules: the spare join a patch is built into (swapped
  // with the bound one on success, so the join's footprint is held twice),
  // the per-slot patch index and keep bitmap over the new rule count, the
  // new degrees, the patch in ascending slot order {patch rule, slot, degree}
  // with its scan, the delta pairs (key0, p_val0) and the removed pairs
  // (p_rkey, p_rval) sorted by node with their node offsets, and the phase
  // events / times of the last patch
  DBuf<int64_t> rn_off2, nt_off2;
  DBuf<int32_t> rn_nodes2, nt_rule2;
  DBuf<int32_t> p_idx, p_deg, p_ord, p_val0;
  DBuf<unsigned long long> p_keep;
  DBuf<int64_t> p_doff, p_dnode_off, p_rem_off;
  DBuf<int32_t> p_rkey, p_rval;
  static constexpr int kPatchPhases = 5;  // join, rule-major, delta sort, removed sort, merge
  hipEvent_t p_ev[kPatchPhases + 1] = {};
  float p_ms[kPatchPhases] = {0, 0, 0, 0, 0};
  void release() {
    rn_off2.release(); nt_off2.release(); rn_nodes2.release(); nt_rule2.release();
    p_idx.release(); p_deg.release(); p_ord.release(); p_val0.release(); p_keep.release();
    p_doff.release(); p_dnode_off.release(); p_rem_off.release(); p_rkey.release(); p_rval.release();
    for (hipEvent_t& e : p_ev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    rn_off.release(); nt_off.release(); rn_nodes.release(); nt_rule.release();
    node_off.release(); slots.release(); tile_cnt.release(); tile_base.release();
    deg.release(); key0.release(); key1.release(); val1.release(); hist.release();
    deg_off.release(); hist_off.release(); scan_tmp.release();
    bound = valid = false;
  }
};

// cg_dispatcher_upcoming* (cg_upcoming.hip): the scratch of the select and the
// last result, in buffers no other entry point touches (a peek leaves the last
// wake, its due list and its fan-out readable).
struct DispatchUpcoming {
  // select: per-block partial histograms (bin-major); their column sums in
  // mapped, coherent pinned memory k_up_colsum stores straight into (no D2H
  // copy launch; read once the stream has drained)
  DBuf<uint32_t> part;
  unsigned long long* totals_host = nullptr;
  unsigned long long* totals_dev = nullptr;
  // compaction: per-tile counts below the cut / inside the cut's class, their scans
  DBuf<int32_t> cnt_lt, cnt_cl;
  DBuf<int64_t> base_lt, base_cl;
  // the selected entries in ascending slot order {key - base, slot}; the sort's
  // 32-bit key chunks and permutation (ping-pong), its histograms
  DBuf<unsigned long long> ckey;
  DBuf<int32_t> cslot, key0, key1, val0, val1, hist;
  DBuf<int64_t> hist_off;
  DBuf<char> scan_tmp;
  // result: n_out entries {slot, Next, Prev} in byTime order
  DBuf<int32_t> slots;
  DBuf<int64_t> next, prev;
  int64_t n_out = 0, n_total = 0;
  bool valid = false;  // a result is readable (cleared by set / remove / fire / patch / bind)
  static constexpr int kPhases = 3;  // select, compaction, sort + gather
  hipEvent_t ev[kPhases + 1] = {};
  float ms[kPhases] = {0, 0, 0};
  int passes = 0;  // streaming passes over the candidates of the last call
  void release() {
    if (totals_host) (void)hipHostFree(totals_host);
    totals_host = totals_dev = nullptr;
    part.release(); cnt_lt.release(); cnt_cl.release(); base_lt.release(); base_cl.release();
    ckey.release(); cslot.release(); key0.release(); key1.release(); val0.release(); val1.release();
    hist.release(); hist_off.release(); scan_tmp.release(); slots.release(); next.release(); prev.release();
    for (hipEvent_t& e : ev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    valid = false;
    n_out = n_total = 0;
  }
};

struct cg_dispatcher {
  cg_ctx* ctx = nullptr;
  cg::ZoneRules zone;
  // slots
  int64_t n = 0;
  size_t cap = 0;  // slots allocated
  cg::DSpec* specs = nullptr;
  int64_t* next = nullptr;
  int64_t* prev = nullptr;
  std::vector<uint8_t> live;
  // wake scratch
  unsigned long long* due_bits = nullptr;
  uint32_t* tile_cnt = nullptr;
  unsigned long long* tile_min = nullptr;
  int32_t* due = nullptr;
  cg::DispatchState* st = nullptr;
  int64_t n_due = 0;
  // due_bits / due hold the last cg_dispatcher_fire's wake (a set or remove
  // since may have reallocated them)
  bool wake_valid = false;
  // the min over Next, host copy (CG_ZERO_TIME = no entry can fire)
  int64_t effective = CG_ZERO_TIME;
  // zone table covering [tab_lo, tab_hi], own buffer (the ctx plan buffer is shared)
  DBuf<char> tab_dev;
  cg::PlanArgs pa{};
  int64_t tab_lo = 1, tab_hi = 0;
  // staging for set/remove
  DBuf<int64_t> idx_dev;
  DBuf<cg::DSpec> src_dev;
  DispatchFanout fo;
  DispatchUpcoming up;

  void release();
  // the zone table for Next walks from `now`
  int ensure_table(int64_t now);
  // every per-slot array sized together, contents of [0, n) kept
  int reserve(int64_t want);
  int reset_state();
  // read the state back; CG_ERANGE if some entry's Next never returns
  int read_state(cg::DispatchState* h);
  int recompute_min();
};
