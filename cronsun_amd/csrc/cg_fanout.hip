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
// cg_dispatcher_patch_rules edits the bound join in place of a rebind (below).
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

// ---- cg_dispatcher_patch_rules: one streaming pass over the bound join ----
// The patch's own join (rule_nodes_locked on the patch) gives the new rows of
// the patched slots.  Rule-major side: new degrees, a scan, a copy of the rows
// from the old join or the patch.  Node-major side: three sorted pieces.  The
// old transpose; the REMOVED pairs, the old rows of the patched slots; the
// DELTA, the patch's rows -- the last two emitted as (node, slot) pairs in
// ascending slot order and sorted stably by node (the transpose's LSD passes;
// both are small).  The survivors are the old pairs of unpatched slots, and
// the new row n is the merge of survivor row n and delta row n, whose slots
// are disjoint.  Nothing is counted or scanned over the old pairs: a survivor
// (n, r) at old position q lands at
//   q - removed pairs before it (those of nodes < n + those of n with a slot < r)
//     + delta pairs before it   (the same two terms)
// and delta pair i = (n, s) at i + the survivors before the first old pair of
// n with a slot above s.  The old transpose is read once and the new one
// written once, in the filter path's tiles, which ignore node boundaries; the
// removed and delta rows a pair ranks into are short and L2-resident, and a
// tile inside one node searches them only between the ranks of its first and
// last pair (equal for most tiles: a shifted copy).

__global__ void k_patch_index(const int32_t* __restrict__ ord_p, const int32_t* __restrict__ ord_slot, int64_t P,
                              int32_t* __restrict__ pidx) {
  const int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (j < P) pidx[ord_slot[j]] = ord_p[j];  // slots are distinct
}

// per slot s < Rn: its new degree, and bit s of keep = s is not patched
__global__ __launch_bounds__(256) void k_patch_deg(const int32_t* __restrict__ pidx, int64_t Rn,
                                                    const int64_t* __restrict__ prn_off,
                                                    const int64_t* __restrict__ rn_off, int64_t R,
                                                    unsigned long long* __restrict__ keep,
                                                    int32_t* __restrict__ deg) {
  const int64_t s = blockIdx.x * int64_t(256) + threadIdx.x;
  const bool in = s < Rn;
  const int32_t p = in ? pidx[s] : 0;
  const unsigned long long m = __ballot(in && p < 0);
  if (!in) return;
  deg[s] = p >= 0 ? int32_t(prn_off[p + 1] - prn_off[p]) : s < R ? int32_t(rn_off[s + 1] - rn_off[s]) : 0;
  if ((threadIdx.x & 63) == 0) keep[s >> 6] = m;
}

// The new rule-major CSR, kPatchRowBlock slots a block.  Where no slot of the
// block is patched (nearly every block of a small patch) the block's rows are
// one contiguous range of the old join that moves by one shift: a flat,
// coalesced copy.  A block with a patched slot, or past the old rule set,
// copies row by row, one wave a row, from the patch or the old join.
constexpr int kPatchRowBlock = 256;

__global__ __launch_bounds__(256) void k_patch_rows(const int32_t* __restrict__ pidx,
                                                     const unsigned long long* __restrict__ keep, int64_t Rn,
                                                     const int64_t* __restrict__ prn_off,
                                                     const int32_t* __restrict__ prn_nodes,
                                                     const int64_t* __restrict__ rn_off,
                                                     const int32_t* __restrict__ rn_nodes, int64_t R,
                                                     const int64_t* __restrict__ new_off,
                                                     int32_t* __restrict__ out) {
  const int64_t s0 = int64_t(blockIdx.x) * kPatchRowBlock, s1 = std::min<int64_t>(s0 + kPatchRowBlock, Rn);
  bool plain = s1 <= R;  // uniform
  for (int64_t w = s0 >> 6; plain && w <= (s1 - 1) >> 6; w++) {
    const int64_t bits = std::min<int64_t>(s1 - w * 64, 64);
    plain = keep[w] == (bits == 64 ? ~0ull : (1ull << bits) - 1ull);
  }
  if (plain) {
    const int64_t a = rn_off[s0], n = rn_off[s1] - a, o = new_off[s0];
#pragma unroll 4
    for (int64_t k = threadIdx.x; k < n; k += 256) out[o + k] = rn_nodes[a + k];
    return;
  }
  const int lane = threadIdx.x & 63;
  for (int64_t s = s0 + (threadIdx.x >> 6); s < s1; s += 4) {
    const int64_t o = new_off[s], n = new_off[s + 1] - o;
    if (n == 0) continue;  // (a slot past the old rule set that is not patched has no row to read)
    const int32_t p = pidx[s];
    const int32_t* src = p >= 0 ? prn_nodes + prn_off[p] : rn_nodes + rn_off[s];
    for (int64_t k = lane; k < n; k += 64) out[o + k] = src[k];
  }
}

// degree of row row_of[j] of a CSR, j-th patched slot in ascending slot order
// (the patch's rows by patch rule, or the old rows by slot: rows >= lim have none)
__global__ void k_patch_ddeg(const int32_t* __restrict__ row_of, int64_t P, const int64_t* __restrict__ off,
                             int64_t lim, int32_t* __restrict__ ddeg) {
  const int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (j < P) ddeg[j] = row_of[j] < lim ? int32_t(off[row_of[j] + 1] - off[row_of[j]]) : 0;
}

// One wave per patched slot: the (node, slot) pairs of its row, slots ascending
__global__ __launch_bounds__(256) void k_patch_pairs(const int32_t* __restrict__ row_of,
                                                      const int32_t* __restrict__ ord_slot, int64_t P,
                                                      const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ nodes, int64_t lim,
                                                      const int64_t* __restrict__ doff,
                                                      uint32_t* __restrict__ key, int32_t* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  for (int64_t j = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < P; j += int64_t(gridDim.x) * 4) {
    if (row_of[j] >= lim) continue;
    const int64_t a = off[row_of[j]], n = off[row_of[j] + 1] - a, o = doff[j];
    const int32_t s = ord_slot[j];
    for (int64_t k = lane; k < n; k += 64) {
      key[o + k] = uint32_t(nodes[a + k]);
      val[o + k] = s;
    }
  }
}

// nt_off of the merged transpose: the old pairs before node v less the removed
// ones, plus the delta pairs (a node past the old set has every old pair before it)
__global__ void k_patch_nt_off(const int64_t* __restrict__ nt_off_old, const int64_t* __restrict__ rem_off,
                               int32_t N, const int64_t* __restrict__ dnode_off, int32_t Nn,
                               int64_t* __restrict__ nt_off) {
  const int64_t v = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (v <= Nn) nt_off[v] = nt_off_old[v <= N ? v : N] - rem_off[v <= N ? v : N] + dnode_off[v];
}

// the largest v in [lo, hi] with off[v] <= q (off[lo] <= q)
__device__ __forceinline__ int32_t last_at_or_before(const int64_t* __restrict__ off, int32_t lo, int32_t hi,
                                                     int64_t q) {
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// first index in [a, b) of the ascending v with v[i] >= x (b: none)
__device__ __forceinline__ int64_t first_at_or_above(const int32_t* __restrict__ v, int64_t a, int64_t b,
                                                     int32_t x) {
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (v[mid] < x) a = mid + 1;
    else b = mid;
  }
  return a;
}

// One tile of the old transpose: every survivor to its place in the new one.
// Threads 0 and 1 rank the tile's first and last pair (node, removed row,
// delta row); every pair then searches between those only.
__global__ __launch_bounds__(256) void k_patch_merge_surv(const int32_t* __restrict__ nt_rule, int64_t nnz,
                                                           const int64_t* __restrict__ nt_off, int32_t N,
                                                           const unsigned long long* __restrict__ keep,
                                                           const int64_t* __restrict__ rem_off,
                                                           const int32_t* __restrict__ rval,
                                                           const int64_t* __restrict__ dnode_off,
                                                           const int32_t* __restrict__ dval,
                                                           int32_t* __restrict__ out) {
  __shared__ int32_t s_node[2];
  __shared__ int64_t s_rem[2], s_del[2];
  const int64_t tile0 = int64_t(blockIdx.x) * kFanTile;
  if (threadIdx.x < 2) {
    const int64_t q = threadIdx.x == 0 ? tile0 : std::min<int64_t>(tile0 + kFanTile, nnz) - 1;
    const int32_t n = last_at_or_before(nt_off, 0, N - 1, q), r = nt_rule[q];
    s_node[threadIdx.x] = n;
    s_rem[threadIdx.x] = first_at_or_above(rval, rem_off[n], rem_off[n + 1], r);
    s_del[threadIdx.x] = first_at_or_above(dval, dnode_off[n], dnode_off[n + 1], r);
  }
  __syncthreads();
  const int32_t n_first = s_node[0], n_last = s_node[1];
  const bool one = n_first == n_last;  // uniform: the tile lies inside one node
  const int64_t rem0 = s_rem[0], rem1 = s_rem[1], del0 = s_del[0], del1 = s_del[1];
  // the tile's loads first, all in flight together
  int32_t r[kFanItems];
  bool kept[kFanItems];
#pragma unroll
  for (int j = 0; j < kFanItems; j++) {
    const int64_t q = tile0 + j * 256 + threadIdx.x;
    r[j] = q < nnz ? nt_rule[q] : -1;
  }
#pragma unroll
  for (int j = 0; j < kFanItems; j++) kept[j] = r[j] >= 0 && due_bit(keep, r[j]);  // else: a patched slot's pair
  if (one && rem0 == rem1 && del0 == del1) {  // uniform: nothing removed or added inside the tile, one shift
    const int64_t o = tile0 + threadIdx.x - rem0 + del0;
#pragma unroll
    for (int j = 0; j < kFanItems; j++)
      if (kept[j]) out[o + j * 256] = r[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < kFanItems; j++) {
    if (!kept[j]) continue;
    const int64_t q = tile0 + j * 256 + threadIdx.x;
    int64_t rem, del;
    if (one) {
      rem = first_at_or_above(rval, rem0, rem1, r[j]);
      del = first_at_or_above(dval, del0, del1, r[j]);
    } else {
      const int32_t n = last_at_or_before(nt_off, n_first, n_last, q);
      rem = first_at_or_above(rval, rem_off[n], rem_off[n + 1], r[j]);
      del = first_at_or_above(dval, dnode_off[n], dnode_off[n + 1], r[j]);
    }
    out[q - rem + del] = r[j];
  }
}

// Delta pair i = (node n, slot s) lands at i + the survivors before the first
// old pair of n with a slot above s.
__global__ void k_patch_merge_delta(const uint32_t* __restrict__ dkey, const int32_t* __restrict__ dval,
                                    int64_t n_delta, const int32_t* __restrict__ nt_rule, int64_t nnz,
                                    const int64_t* __restrict__ nt_off, int32_t N,
                                    const int64_t* __restrict__ rem_off, const int32_t* __restrict__ rval,
                                    int32_t* __restrict__ out) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n_delta) return;
  const int32_t n = int32_t(dkey[i]), s = dval[i];
  int64_t before = nnz - rem_off[N];  // a node past the old set: every survivor comes first
  if (n < N)
    before = first_at_or_above(nt_rule, nt_off[n], nt_off[n + 1], s) -
             first_at_or_above(rval, rem_off[n], rem_off[n + 1], s);
  out[i + before] = s;
}

struct SlotOf {
  int64_t slot;
  int32_t p;
};

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
  d->up.valid = false;
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
  f.mode = mode;
  f.bound = true;
  return CG_OK;
}

int cg_dispatcher_patch_rules(cg_dispatcher* d, const cg_rules* patch, const int64_t* slot) {
  if (!d || !patch) return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: null");
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  DispatchFanout& f = d->fo;
  if (!f.bound)
    return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: no rule set bound (cg_dispatcher_bind_rules)");
  if (patch->ctx != c) return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: patch uploaded on another context");
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  if (async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined rule-major calls pending (call cg_expand_wait first)");
  const RulesStore& st = patch->st;
  const int64_t P = st.n_rules;
  if (P == 0) return CG_OK;
  d->up.valid = false;  // (a per-node list describes the join this patch edits)
  if (!slot) return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: null slots");
  // the patch in ascending slot order (the delta pairs are emitted in it)
  std::vector<SlotOf> ord(size_t(P), SlotOf{0, 0});
  for (int64_t p = 0; p < P; p++) {
    if (slot[p] < 0 || slot[p] >= d->n)
      return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: slot " + std::to_string(slot[p]) + " of patch rule " +
                                    std::to_string(p) + " outside the dispatcher's " + std::to_string(d->n) +
                                    " slots");
    ord[size_t(p)] = SlotOf{slot[p], int32_t(p)};
  }
  std::sort(ord.begin(), ord.end(), [](const SlotOf& a, const SlotOf& b) { return a.slot < b.slot; });
  for (int64_t j = 1; j < P; j++)
    if (ord[size_t(j)].slot == ord[size_t(j - 1)].slot)
      return cg_fail(CG_EINVAL, "cg_dispatcher_patch_rules: slot " + std::to_string(ord[size_t(j)].slot) +
                                    " appears twice (patch rules " + std::to_string(ord[size_t(j - 1)].p) +
                                    " and " + std::to_string(ord[size_t(j)].p) + ")");
  const int64_t R = f.R, Rn = std::max(R, ord.back().slot + 1), nnz = f.nnz;
  const int32_t N = f.N, Nn = std::max(N, st.n_nodes);
  std::vector<int32_t> h_ord(size_t(2 * P));  // [patch rule | slot]
  for (int64_t j = 0; j < P; j++) {
    h_ord[size_t(j)] = ord[size_t(j)].p;
    h_ord[size_t(P + j)] = int32_t(ord[size_t(j)].slot);
  }
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  for (hipEvent_t& e : f.p_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  hipStream_t s = c->st;
  // The patch's join, in the ctx's shared buffers (c->rn_off, c->rn_nodes):
  // the per-node path caches those by rule set and mode, so drop that cache.
  c->pn_cache_serial = 0;
  (void)hipEventRecord(f.p_ev[0], s);
  int64_t pnnz = 0;
  int rc = rule_nodes_locked(c, st, f.mode, &pnnz);
  if (rc) return rc;
  (void)hipEventRecord(f.p_ev[1], s);
  // Everything below writes only the spare join and scratch: the bound join
  // stays what it was until the swap at the end.
  const size_t tmp = std::max(scan_temp_bytes(Rn), scan_temp_bytes(P));
  // a new allocation of a spare pair array takes 1/16 more than the new pair
  // total, so a run of patches that each add a little does not reallocate
  auto spare = [](DBuf<int32_t>& b, int64_t n) {
    return size_t(n) <= b.cap ? CG_OK : b.ensure(size_t(n + n / 16 + 1));
  };
  if ((rc = f.rn_off2.ensure(size_t(Rn) + 1)) || (rc = f.nt_off2.ensure(size_t(Nn) + 1)) ||
      (rc = f.p_idx.ensure(size_t(Rn))) || (rc = f.p_deg.ensure(size_t(Rn))) ||
      (rc = f.p_keep.ensure(size_t((Rn + 63) / 64))) ||
      (rc = f.p_ord.ensure(size_t(3 * P))) || (rc = f.p_doff.ensure(size_t(P) + 1)) ||
      (rc = f.p_dnode_off.ensure(size_t(Nn) + 1)) || (rc = f.p_rem_off.ensure(size_t(N) + 1)) ||
      (rc = f.scan_tmp.ensure(std::max(f.scan_tmp.cap, tmp))))
    return rc;
  const int32_t *ord_p = f.p_ord.p, *ord_slot = f.p_ord.p + P;
  int32_t* ddeg = f.p_ord.p + 2 * P;
  const int64_t* prn_off = c->rn_off.p;
  const int32_t* prn_nodes = c->rn_nodes.p;
  HIPCHK(hipMemcpyAsync(f.p_ord.p, h_ord.data(), size_t(2 * P) * 4, hipMemcpyHostToDevice, s));
  // rule-major side
  HIPCHK(hipMemsetAsync(f.p_idx.p, 0xFF, size_t(Rn) * 4, s));
  hipLaunchKernelGGL(k_patch_index, dim3(grid_of(P, 256, int64_t(1) << 30)), dim3(256), 0, s, ord_p, ord_slot, P,
                     f.p_idx.p);
  hipLaunchKernelGGL(k_patch_deg, dim3(grid_of(Rn, 256, int64_t(1) << 30)), dim3(256), 0, s, f.p_idx.p, Rn,
                     prn_off, f.rn_off.p, R, f.p_keep.p, f.p_deg.p);
  launch_scan(f.p_deg.p, f.rn_off2.p, Rn, f.scan_tmp.p, s);
  HIPCHK(hipGetLastError());
  // the new pair total sizes the spare pair arrays and gives the removed
  // pairs (the old rows of the patched slots)
  int64_t nnz_new = 0;
  if ((rc = read_i64(c, f.rn_off2.p + Rn, &nnz_new))) return rc;
  const int64_t rnnz = nnz + pnnz - nnz_new;
  if ((rc = spare(f.rn_nodes2, std::max<int64_t>(nnz_new, 1))) ||
      (rc = spare(f.nt_rule2, std::max<int64_t>(nnz_new, 1))))
    return rc;
  hipLaunchKernelGGL(k_patch_rows, dim3(grid_of(Rn, kPatchRowBlock, int64_t(1) << 30)), dim3(256), 0, s,
                     f.p_idx.p, f.p_keep.p, Rn, prn_off, prn_nodes, f.rn_off.p, f.rn_nodes.p, R, f.rn_off2.p,
                     f.rn_nodes2.p);
  (void)hipEventRecord(f.p_ev[2], s);
  HIPCHK(hipGetLastError());
  // the delta and the removed pairs, each in ascending slot order, sorted stably by node
  auto sorted_pairs = [&](const int32_t* row_of, const int64_t* off, const int32_t* nodes, int64_t lim, int64_t n,
                          int32_t Nk, DBuf<int32_t>& k0, DBuf<int32_t>& v0, int64_t* node_off) -> int {
    if (n == 0) return cg_hip_check(hipMemsetAsync(node_off, 0, size_t(Nk + 1) * 8, s), "hipMemset");
    const int64_t hw = radix_hist_words(n);
    int rc2;
    if ((rc2 = k0.ensure(size_t(n))) || (rc2 = v0.ensure(size_t(n))) || (rc2 = f.key1.ensure(size_t(n))) ||
        (rc2 = f.val1.ensure(size_t(n))) || (rc2 = f.hist.ensure(size_t(hw))) ||
        (rc2 = f.hist_off.ensure(size_t(hw) + 1)) ||
        (rc2 = f.scan_tmp.ensure(std::max(f.scan_tmp.cap, scan_temp_bytes(hw)))))
      return rc2;
    hipLaunchKernelGGL(k_patch_ddeg, dim3(grid_of(P, 256, int64_t(1) << 30)), dim3(256), 0, s, row_of, P, off, lim,
                       ddeg);
    launch_scan(ddeg, f.p_doff.p, P, f.scan_tmp.p, s);
    hipLaunchKernelGGL(k_patch_pairs, dim3(grid_of(P, 4, 256 * 64)), dim3(256), 0, s, row_of, ord_slot, P, off,
                       nodes, lim, f.p_doff.p, reinterpret_cast<uint32_t*>(k0.p), v0.p);
    bool in_second = false;
    radix_by_key_enqueue(s, reinterpret_cast<uint32_t*>(k0.p), v0.p, reinterpret_cast<uint32_t*>(f.key1.p),
                         f.val1.p, n, Nk, f.hist.p, f.hist_off.p, f.scan_tmp.p, &in_second);
    if (in_second) {  // keep the sorted pairs in (k0, v0)
      std::swap(k0, f.key1);
      std::swap(v0, f.val1);
    }
    launch_node_bounds(s, reinterpret_cast<const uint32_t*>(k0.p), n, Nk, node_off);
    return cg_hip_check(hipGetLastError(), "patch pairs");
  };
  if ((rc = sorted_pairs(ord_p, prn_off, prn_nodes, P, pnnz, Nn, f.key0, f.p_val0, f.p_dnode_off.p))) return rc;
  (void)hipEventRecord(f.p_ev[3], s);
  if ((rc = sorted_pairs(ord_slot, f.rn_off.p, f.rn_nodes.p, R, rnnz, N, f.p_rkey, f.p_rval, f.p_rem_off.p)))
    return rc;
  hipLaunchKernelGGL(k_patch_nt_off, dim3(grid_of(int64_t(Nn) + 1, 256, int64_t(1) << 30)), dim3(256), 0, s,
                     f.nt_off.p, f.p_rem_off.p, N, f.p_dnode_off.p, Nn, f.nt_off2.p);
  (void)hipEventRecord(f.p_ev[4], s);
  // the merge
  if (nnz > 0)
    hipLaunchKernelGGL(k_patch_merge_surv, dim3(unsigned((nnz + kFanTile - 1) / kFanTile)), dim3(256), 0, s,
                       f.nt_rule.p, nnz, f.nt_off.p, N, f.p_keep.p, f.p_rem_off.p, f.p_rval.p, f.p_dnode_off.p,
                       f.p_val0.p, f.nt_rule2.p);
  if (pnnz > 0)
    hipLaunchKernelGGL(k_patch_merge_delta, dim3(grid_of(pnnz, 256, int64_t(1) << 30)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(f.key0.p), f.p_val0.p, pnnz, f.nt_rule.p, nnz, f.nt_off.p,
                       N, f.p_rem_off.p, f.p_rval.p, f.nt_rule2.p);
  (void)hipEventRecord(f.p_ev[5], s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  for (int i = 0; i < DispatchFanout::kPatchPhases; i++)
    (void)hipEventElapsedTime(&f.p_ms[i], f.p_ev[i], f.p_ev[i + 1]);
  std::swap(f.rn_off, f.rn_off2);
  std::swap(f.rn_nodes, f.rn_nodes2);
  std::swap(f.nt_off, f.nt_off2);
  std::swap(f.nt_rule, f.nt_rule2);
  f.R = Rn;
  f.N = Nn;
  f.nnz = nnz_new;
  // the wake stands (its due list is untouched); its fan-out under the old join does not
  f.valid = false;
  f.n_pairs = 0;
  return CG_OK;
}

int cg_dispatcher_patch_times(const cg_dispatcher* d, float* ms, int n) {
  if (!d || !ms || n < 0) return cg_fail(CG_EINVAL, "cg_dispatcher_patch_times: null");
  std::lock_guard<std::mutex> g(d->ctx->mu);
  const int k = std::min(n, DispatchFanout::kPatchPhases);
  for (int i = 0; i < k; i++) ms[i] = d->fo.p_ms[i];
  return k;
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
  c->kt[KT_FANOUT] = 0.f;
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
  (void)hipEventElapsedTime(&c->kt[KT_FANOUT], c->pev[0], c->pev[1]);
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
