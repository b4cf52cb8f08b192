// cg_fanout.hip -- node fan-out of a dispatcher wake on gfx950: which node
// runs which of the due entries.
//
// One dispatcher table holds every rule of the cluster (slot i = rule i of a
// bound cg_rules).  In the reference every cronnode runs its own Cron over
// its own Cmds (node/node.go:121-158, node/cron/cron.go:210-275); the fan-out
// of a wake is what those N run loops fire at that instant: a node-major CSR
// of the due slots, slots ascending within a node, over the same rule -> node
// join the per-node batch path uses (rule_nodes_locked / transpose_locked).
//
// Two device paths, one result:
//   filter (dense wakes)   the node-major transpose nt_rule already is the
//     answer for "everything due": the fan-out is its ordered compaction by
//     the wake's due bitmap (k_dispatch_scan leaves one bit per entry,
//     L2-resident).  k_fan_count counts the due pairs of every 2048-pair tile
//     of nt_rule, the scan turns the counts into tile bases, k_fan_write
//     compacts each tile with wave ballots + prefix popcounts, and
//     k_fan_node_off ranks every node's first pair (nt_off[n]) among the due
//     pairs: node_off[n] = tile base + the due pairs of the tile before it.
//     Tiles ignore node boundaries, so one dense node spreads over the grid;
//     no atomics, no sort.
//   due-driven (sparse wakes)   the degree of every due slot from rn_off, a
//     scan, the (node, slot) pairs in due order, the transpose's stable LSD
//     passes by node (slots stay ascending within a node), k_node_bounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "cg_api_internal.h"
#include "cg_dispatcher.h"

using namespace cg;

namespace {

constexpr int kFanItems = 8;
constexpr int kFanTile = 256 * kFanItems;  // pairs of nt_rule per block
constexpr int kFanWave = 64 * kFanItems;   // pairs per wave: item j = its pairs [j*64, j*64+64)

// AUTO takes the due-driven path when the pairs it expects, n_due * nnz /
// n_rules, times this factor stay below nnz (what the filter path streams
// whatever the wake).  Measured crossover: DESIGN.md, "Dispatcher fan-out".
constexpr int64_t kFanDueFactor = 12;

__device__ __forceinline__ bool due_bit(const unsigned long long* __restrict__ due_bits, int32_t r) {
  return (due_bits[r >> 6] >> (r & 63)) & 1ull;
}

// the wave's kFanItems ballots of tile b: bit l of m[j] = pair base + j*64 + l is due
__device__ __forceinline__ void fan_ballots(const int32_t* __restrict__ nt_rule, int64_t nnz,
                                            const unsigned long long* __restrict__ due_bits, int64_t base,
                                            int lane, int32_t (&r)[kFanItems], unsigned long long (&m)[kFanItems]) {
#pragma unroll
  for (int j = 0; j < kFanItems; j++) {
    const int64_t p = base + j * 64 + lane;
    r[j] = p < nnz ? nt_rule[p] : -1;
  }
#pragma unroll
  for (int j = 0; j < kFanItems; j++) m[j] = __ballot(r[j] >= 0 && due_bit(due_bits, r[j]));
}

__global__ __launch_bounds__(256) void k_fan_count(const int32_t* __restrict__ nt_rule, int64_t nnz,
                                                    const unsigned long long* __restrict__ due_bits,
                                                    int32_t* __restrict__ tile_cnt) {
  __shared__ int32_t s_cnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t r[kFanItems];
  unsigned long long m[kFanItems];
  fan_ballots(nt_rule, nnz, due_bits, int64_t(blockIdx.x) * kFanTile + wv * kFanWave, lane, r, m);
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kFanItems; j++) c += __popcll(m[j]);
  if (lane == 0) s_cnt[wv] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(256) void k_fan_write(const int32_t* __restrict__ nt_rule, int64_t nnz,
                                                    const unsigned long long* __restrict__ due_bits,
                                                    const int64_t* __restrict__ tile_base,
                                                    int32_t* __restrict__ slots) {
  __shared__ int32_t s_cnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t lo = tile_base[blockIdx.x];
  if (tile_base[blockIdx.x + 1] == lo) return;  // uniform: nothing due in this tile
  int32_t r[kFanItems];
  unsigned long long m[kFanItems];
  fan_ballots(nt_rule, nnz, due_bits, int64_t(blockIdx.x) * kFanTile + wv * kFanWave, lane, r, m);
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kFanItems; j++) c += __popcll(m[j]);
  if (lane == 0) s_cnt[wv] = c;
  __syncthreads();
  int64_t o = lo;
  for (int w = 0; w < wv; w++) o += s_cnt[w];
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kFanItems; j++) {
    if ((m[j] >> lane) & 1ull) slots[o + __popcll(m[j] & lt)] = r[j];
    o += __popcll(m[j]);
  }
}

// One wave per node v in [0, N]: node_off[v] = due pairs before position
// nt_off[v] of the transpose = its tile's base + the due pairs of the tile
// before it (at most kFanTile / 64 ballots).
__global__ __launch_bounds__(256) void k_fan_node_off(const int64_t* __restrict__ nt_off, int32_t N,
                                                       const int32_t* __restrict__ nt_rule, int64_t nnz,
                                                       const unsigned long long* __restrict__ due_bits,
                                                       const int64_t* __restrict__ tile_base,
                                                       int64_t* __restrict__ node_off) {
  const int lane = threadIdx.x & 63;
  const int64_t v = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (v > N) return;  // uniform per wave
  const int64_t p = nt_off[v];
  const int64_t t = p / kFanTile;  // (p == nnz on a tile edge: t = tiles, tile_base[tiles] = the total)
  int64_t c = 0;
  for (int64_t q = t * kFanTile + lane; q - lane < p; q += 64) {
    const bool due = q < p && due_bit(due_bits, nt_rule[q]);
    c += __popcll(__ballot(due));
  }
  if (lane == 0) node_off[v] = tile_base[t] + c;
}

// deg[j] = nodes of due slot j (a slot past the bound rule set has none)
__global__ void k_fan_deg(const int32_t* __restrict__ due, int64_t n_due, const int64_t* __restrict__ rn_off,
                          int64_t R, int32_t* __restrict__ deg) {
  const int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (j >= n_due) return;
  const int64_t s = due[j];
  deg[j] = s < R ? int32_t(rn_off[s + 1] - rn_off[s]) : 0;
}

// One wave per due slot: its (node, slot) pairs, in due order
__global__ __launch_bounds__(256) void k_fan_pairs(const int32_t* __restrict__ due, int64_t n_due,
                                                    const int64_t* __restrict__ rn_off,
                                                    const int32_t* __restrict__ rn_nodes, int64_t R,
                                                    const int64_t* __restrict__ deg_off,
                                                    uint32_t* __restrict__ key, int32_t* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  for (int64_t j = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < n_due; j += int64_t(gridDim.x) * 4) {
    const int32_t s = due[j];
    if (s >= R) continue;
    const int64_t a = rn_off[s], n = rn_off[s + 1] - a, o = deg_off[j];
    for (int64_t k = lane; k < n; k += 64) {
      key[o + k] = uint32_t(rn_nodes[a + k]);
      val[o + k] = s;
    }
  }
}

int grid_of(int64_t n, int per_block, int64_t cap) {
  return int(std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, cap)));
}

int read_i64(cg_ctx* c, const int64_t* dev, int64_t* out) {
  HIPCHK(hipMemcpyAsync(out, dev, 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

int fan_filter(cg_dispatcher* d) {
  cg_ctx* c = d->ctx;
  DispatchFanout& f = d->fo;
  const int64_t tiles = (f.nnz + kFanTile - 1) / kFanTile;
  int rc;
  if ((rc = f.tile_cnt.ensure(size_t(tiles))) || (rc = f.tile_base.ensure(size_t(tiles) + 1)) ||
      (rc = f.scan_tmp.ensure(scan_temp_bytes(tiles))))
    return rc;
  hipLaunchKernelGGL(k_fan_count, dim3(unsigned(tiles)), dim3(256), 0, c->st, f.nt_rule.p, f.nnz, d->due_bits,
                     f.tile_cnt.p);
  launch_scan(f.tile_cnt.p, f.tile_base.p, tiles, f.scan_tmp.p, c->st);
  HIPCHK(hipGetLastError());
  int64_t total = 0;
  if ((rc = read_i64(c, f.tile_base.p + tiles, &total))) return rc;
  if ((rc = f.slots.ensure(size_t(std::max<int64_t>(total, 1))))) return rc;
  if (total > 0)
    hipLaunchKernelGGL(k_fan_write, dim3(unsigned(tiles)), dim3(256), 0, c->st, f.nt_rule.p, f.nnz, d->due_bits,
                       f.tile_base.p, f.slots.p);
  hipLaunchKernelGGL(k_fan_node_off, dim3(unsigned((int64_t(f.N) + 1 + 3) / 4)), dim3(256), 0, c->st, f.nt_off.p,
                     f.N, f.nt_rule.p, f.nnz, d->due_bits, f.tile_base.p, f.node_off.p);
  HIPCHK(hipGetLastError());
  f.n_pairs = total;
  return CG_OK;
}

int fan_due(cg_dispatcher* d) {
  cg_ctx* c = d->ctx;
  DispatchFanout& f = d->fo;
  const int64_t nd = d->n_due;
  int rc;
  if ((rc = f.deg.ensure(size_t(nd))) || (rc = f.deg_off.ensure(size_t(nd) + 1)) ||
      (rc = f.scan_tmp.ensure(scan_temp_bytes(nd))))
    return rc;
  hipLaunchKernelGGL(k_fan_deg, dim3(grid_of(nd, 256, int64_t(1) << 30)), dim3(256), 0, c->st, d->due, nd,
                     f.rn_off.p, f.R, f.deg.p);
  launch_scan(f.deg.p, f.deg_off.p, nd, f.scan_tmp.p, c->st);
  HIPCHK(hipGetLastError());
  int64_t total = 0;
  if ((rc = read_i64(c, f.deg_off.p + nd, &total))) return rc;
  f.n_pairs = total;
  if (total == 0) return cg_hip_check(hipMemsetAsync(f.node_off.p, 0, size_t(f.N + 1) * 8, c->st), "hipMemset");
  const size_t cap = size_t(total);
  const int64_t hw = radix_hist_words(total);
  if ((rc = f.slots.ensure(cap)) || (rc = f.val1.ensure(cap)) || (rc = f.key0.ensure(cap)) ||
      (rc = f.key1.ensure(cap)) || (rc = f.hist.ensure(size_t(hw))) || (rc = f.hist_off.ensure(size_t(hw) + 1)) ||
      (rc = f.scan_tmp.ensure(std::max(f.scan_tmp.cap, scan_temp_bytes(hw)))))
    return rc;
  hipLaunchKernelGGL(k_fan_pairs, dim3(grid_of(nd, 4, 256 * 64)), dim3(256), 0, c->st, d->due, nd, f.rn_off.p,
                     f.rn_nodes.p, f.R, f.deg_off.p, reinterpret_cast<uint32_t*>(f.key0.p), f.slots.p);
  bool in_second = false;
  radix_by_key_enqueue(c->st, reinterpret_cast<uint32_t*>(f.key0.p), f.slots.p,
                       reinterpret_cast<uint32_t*>(f.key1.p), f.val1.p, total, f.N, f.hist.p, f.hist_off.p,
                       f.scan_tmp.p, &in_second);
  if (in_second) {  // keep the sorted pairs in (key0, slots)
    std::swap(f.key0, f.key1);
    std::swap(f.slots, f.val1);
  }
  launch_node_bounds(c->st, reinterpret_cast<const uint32_t*>(f.key0.p), total, f.N, f.node_off.p);
  return cg_hip_check(hipGetLastError(), "fan-out (due-driven)");
}

}  // namespace

extern "C" {

int cg_dispatcher_bind_rules(cg_dispatcher* d, const cg_rules* rules, int mode) {
  if (!d || !rules) return cg_fail(CG_EINVAL, "cg_dispatcher_bind_rules: null");
  cg_ctx* c = d->ctx;
  if (rules->ctx != c) return cg_fail(CG_EINVAL, "rule set uploaded on another context");
  if (mode < 0 || mode > 2) return cg_fail(CG_EINVAL, "bad exclude mode");
  std::lock_guard<std::mutex> g(c->mu);
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  if (async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined rule-major calls pending (call cg_expand_wait first)");
  const RulesStore& st = rules->st;
  if (d->n < int64_t(st.n_rules))
    return cg_fail(CG_EINVAL, "cg_dispatcher_bind_rules: the dispatcher has " + std::to_string(d->n) +
                                  " slots, the rule set " + std::to_string(st.n_rules) + " rules");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  DispatchFanout& f = d->fo;
  f.bound = f.valid = false;
  // The join is built in the ctx's shared buffers, which the per-node path
  // caches by rule set and mode: drop that cache, then move the result out
  // (rn_nodes is copied before the transpose consumes it).
  c->pn_cache_serial = 0;
  int64_t nnz = 0;
  int rc = rule_nodes_locked(c, st, mode, &nnz);
  if (rc) return rc;
  if ((rc = f.rn_nodes.ensure(size_t(std::max<int64_t>(nnz, 1))))) return rc;
  if (nnz)
    HIPCHK(hipMemcpyAsync(f.rn_nodes.p, c->rn_nodes.p, size_t(nnz) * 4, hipMemcpyDeviceToDevice, c->st));
  if ((rc = transpose_locked(c, nnz, st.n_nodes))) return rc;
  HIPCHK(hipStreamSynchronize(c->st));
  std::swap(f.rn_off, c->rn_off);
  std::swap(f.nt_off, c->nt_off);
  std::swap(f.nt_rule, c->nt_rule);
  f.N = st.n_nodes;
  f.R = st.n_rules;
  f.nnz = nnz;
  f.n_pairs = 0;
  f.bound = true;
  return CG_OK;
}

int cg_dispatcher_set_fanout_path(cg_dispatcher* d, int path) {
  if (!d) return cg_fail(CG_EINVAL, "cg_dispatcher_set_fanout_path: null");
  if (path != CG_FANOUT_AUTO && path != CG_FANOUT_FILTER && path != CG_FANOUT_DUE)
    return cg_fail(CG_EINVAL, "cg_dispatcher_set_fanout_path: bad path");
  std::lock_guard<std::mutex> g(d->ctx->mu);
  d->fo.path = path;
  return CG_OK;
}

int cg_dispatcher_fanout(cg_dispatcher* d, int64_t* n_pairs) {
  if (!d || !n_pairs) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout: null");
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  DispatchFanout& f = d->fo;
  *n_pairs = 0;
  if (!f.bound) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout: no rule set bound (cg_dispatcher_bind_rules)");
  if (!d->wake_valid)
    return cg_fail(CG_EINVAL, "cg_dispatcher_fanout: no wake since the last set / remove (the due list is gone)");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  f.valid = false;
  f.n_pairs = 0;
  c->kt[13] = 0.f;
  int rc = f.node_off.ensure(size_t(f.N) + 1);
  if (rc) return rc;
  if (d->n_due == 0 || f.nnz == 0) {
    HIPCHK(hipMemsetAsync(f.node_off.p, 0, size_t(f.N + 1) * 8, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    f.valid = true;
    return CG_OK;
  }
  int path = f.path;
  if (path == CG_FANOUT_AUTO) {
    // expected pairs of the wake from what the host holds: n_due * nnz / R
    const double est = double(d->n_due) * double(f.nnz) / double(std::max<int64_t>(f.R, 1));
    path = est * double(kFanDueFactor) < double(f.nnz) ? CG_FANOUT_DUE : CG_FANOUT_FILTER;
  }
  (void)hipEventRecord(c->pev[0], c->st);
  rc = path == CG_FANOUT_DUE ? fan_due(d) : fan_filter(d);
  if (rc) return rc;
  (void)hipEventRecord(c->pev[1], c->st);
  HIPCHK(hipStreamSynchronize(c->st));
  (void)hipEventElapsedTime(&c->kt[13], c->pev[0], c->pev[1]);
  f.valid = true;
  *n_pairs = f.n_pairs;
  return CG_OK;
}

int cg_dispatcher_fanout_copy(const cg_dispatcher* d, int64_t* node_off, int32_t* slots, int64_t cap) {
  if (!d) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_copy: null");
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  const DispatchFanout& f = d->fo;
  if (!f.valid) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_copy: no fan-out of the last wake");
  if (slots && cap < f.n_pairs)
    return cg_fail(CG_ECAPACITY, "cg_dispatcher_fanout_copy: slots buffer too small, " +
                                     std::to_string(f.n_pairs) + " pairs required");
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  if (node_off)
    HIPCHK(hipMemcpyAsync(node_off, f.node_off.p, size_t(f.N + 1) * 8, hipMemcpyDeviceToHost, c->st));
  if (slots && f.n_pairs)
    HIPCHK(hipMemcpyAsync(slots, f.slots.p, size_t(f.n_pairs) * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

int cg_dispatcher_fanout_range(const cg_dispatcher* d, int64_t first, int64_t count, int32_t* slots) {
  if (!d || (count && !slots)) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_range: null");
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  const DispatchFanout& f = d->fo;
  if (!f.valid) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_range: no fan-out of the last wake");
  if (first < 0 || count < 0 || first + count > f.n_pairs)
    return cg_fail(CG_ERANGE, "cg_dispatcher_fanout_range: range outside the last fan-out");
  if (!count) return CG_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(slots, f.slots.p + first, size_t(count) * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

int cg_dispatcher_fanout_device(const cg_dispatcher* d, const int64_t** d_node_off, const int32_t** d_slots,
                                int64_t* n_pairs) {
  if (!d) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_device: null");
  std::lock_guard<std::mutex> g(d->ctx->mu);
  const DispatchFanout& f = d->fo;
  if (!f.valid) return cg_fail(CG_EINVAL, "cg_dispatcher_fanout_device: no fan-out of the last wake");
  if (d_node_off) *d_node_off = f.node_off.p;
  if (d_slots) *d_slots = f.slots.p;
  if (n_pairs) *n_pairs = f.n_pairs;
  return CG_OK;
}

}  // extern "C"
