// cg_top_rules.hip -- top rules of a profile bucket: for every row (a node of
// the last per-node profile, or the one cluster-wide row of all rules) the k
// largest cells of one column of the rule matrix among the row's rules,
// ordered by (count descending, rule index ascending) ("top
// rules").  Everything it reads is in HBM after a profile call: the rule
// matrix (pf_rules), the node-major transpose (nt_off / nt_rule) and its cut
// into chunks of kNodeChunk rules (pf_chunk_off).
//
//   k_top_select  one wave per chunk of a row's rule list: one pass over the
//                 (row, rule) pairs, one gathered cell per pair.  The wave
//                 keeps its best 64 candidates in registers, one per lane,
//                 sorted; a ballot against the k-th finds the candidates of a
//                 batch that enter, each is placed by a one-lane shift.  A row
//                 of one chunk is finished here, a split row leaves its
//                 chunk's list and non-zero count
//   k_top_merge   one block per split row: the same selection over the row's
//                 chunk lists, the four waves' lists merged through LDS
//
// A candidate is the 64-bit key (cell << 32) | ~rule: larger is better, keys
// of one row are distinct, and 0 (no candidate; a zero cell is never listed)
// loses to all.  So the order of the result does not depend on the order the
// candidates arrive in, every output word is stored once and no atomics are
// used.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"

namespace {

using u64 = unsigned long long;

static_assert(CG_TOP_RULES_MAX == 64, "one list entry per lane of a wave");
static_assert(kNodeChunk % 64 == 0, "whole batches per chunk");

__device__ __forceinline__ u64 shfl64(u64 x, int src) {
  const int32_t lo = __shfl(int32_t(uint32_t(x)), src, 64), hi = __shfl(int32_t(uint32_t(x >> 32)), src, 64);
  return (u64(uint32_t(hi)) << 32) | uint32_t(lo);
}
__device__ __forceinline__ u64 shfl_up64(u64 x) {
  const int32_t lo = __shfl_up(int32_t(uint32_t(x)), 1, 64), hi = __shfl_up(int32_t(uint32_t(x >> 32)), 1, 64);
  return (u64(uint32_t(hi)) << 32) | uint32_t(lo);
}

__device__ __forceinline__ u64 top_key(int32_t cell, int32_t rule) {
  return cell > 0 ? (u64(uint32_t(cell)) << 32) | uint32_t(~rule) : 0;
}

// The wave's list: lane i holds the i-th best key seen so far (0: none), thr
// is the k-th (lane k-1): only a key above it can enter the first k.  One
// batch of up to 64 candidates, one per lane (0: none): those above thr are
// inserted one after the other (thr rises as they are, so a later one of the
// batch is tested again).  All lanes of the wave call this together.
__device__ __forceinline__ void top_insert(u64 key, u64& held, u64& thr, int32_t k, int32_t lane) {
  u64 m = __ballot(key > thr);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const u64 ck = shfl64(key, src);
    if (ck <= thr) continue;  // (wave-uniform)
    const int32_t pos = __popcll(__ballot(held > ck));  // the list is sorted: lanes [0, pos) stay
    const u64 up = shfl_up64(held);
    held = lane < pos ? held : (lane == pos ? ck : up);
    thr = shfl64(held, k - 1);
  }
}

// a finished row: the first k of the list, then padding (-1, 0)
__device__ __forceinline__ void top_store_row(int64_t row, u64 held, int32_t nz, int32_t k, int32_t lane,
                                              int32_t* __restrict__ out_rule, int32_t* __restrict__ out_cnt,
                                              int32_t* __restrict__ out_nl, int32_t* __restrict__ out_nc) {
  if (lane < k) {
    out_rule[row * k + lane] = held ? int32_t(~uint32_t(held)) : -1;
    out_cnt[row * k + lane] = int32_t(held >> 32);
  }
  if (lane == 0) {
    out_nc[row] = nz;
    out_nl[row] = nz < k ? nz : k;
  }
}

__device__ __forceinline__ int32_t wave_sum(int32_t x) {
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// Wave (4 * blockIdx.x + wave) takes chunk ch.  nt_rule != null: chunk ch of
// the nodes' rule lists (chunk_off [N+1], as k_profile_nodes); null: the one
// row of rules [0, R1), chunk ch = rules [ch * kNodeChunk, ...).  Row n ranks
// column bucket[n] of rc [R][B]; the cell index is formed in 64 bits.
__global__ __launch_bounds__(256) void k_top_select(const int64_t* __restrict__ nt_off,
                                                     const int32_t* __restrict__ nt_rule,
                                                     const int64_t* __restrict__ chunk_off, int32_t N, int64_t R1,
                                                     const int32_t* __restrict__ rc, int32_t B,
                                                     const int32_t* __restrict__ bucket, int32_t k,
                                                     int32_t* __restrict__ out_rule, int32_t* __restrict__ out_cnt,
                                                     int32_t* __restrict__ out_nl, int32_t* __restrict__ out_nc,
                                                     u64* __restrict__ part, int32_t* __restrict__ part_nz) {
  const int32_t lane = threadIdx.x & 63;
  const int64_t ch = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  int32_t n = 0;
  int64_t nch, beg, end;
  if (nt_rule) {
    if (ch >= chunk_off[N]) return;  // a whole wave
    // the node of chunk ch: the last n with chunk_off[n] <= ch
    int32_t n0 = 0, n1 = N - 1;
    while (n0 < n1) {
      const int32_t mid = (n0 + n1 + 1) >> 1;
      if (chunk_off[mid] <= ch) n0 = mid;
      else n1 = mid - 1;
    }
    n = n0;
    const int64_t c0 = chunk_off[n], lend = nt_off[n + 1];
    nch = chunk_off[n + 1] - c0;
    beg = nt_off[n] + (ch - c0) * kNodeChunk;
    end = beg + kNodeChunk < lend ? beg + kNodeChunk : lend;
  } else {
    nch = R1 <= kNodeChunk ? 1 : (R1 + kNodeChunk - 1) / kNodeChunk;
    if (ch >= nch) return;
    beg = ch * kNodeChunk;
    end = beg + kNodeChunk < R1 ? beg + kNodeChunk : R1;
  }
  const int64_t col = bucket[n];
  u64 held = 0, thr = 0;
  int32_t nz = 0;
  // four batches a round: the four rule reads, then the four gathers, are in
  // flight together before the first candidate is looked at
  for (int64_t j0 = beg + lane; j0 - lane < end; j0 += 256) {
    int32_t rule[4], cell[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t j = j0 + 64 * u;
      rule[u] = j < end ? (nt_rule ? nt_rule[j] : int32_t(j)) : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) cell[u] = rule[u] >= 0 ? rc[int64_t(rule[u]) * B + col] : 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      nz += cell[u] > 0;
      top_insert(top_key(cell[u], rule[u]), held, thr, k, lane);
    }
  }
  nz = wave_sum(nz);
  if (nch == 1) {
    top_store_row(n, held, nz, k, lane, out_rule, out_cnt, out_nl, out_nc);
  } else {
    if (lane < k) part[ch * k + lane] = held;
    if (lane == 0) part_nz[ch] = nz;
  }
}

// block n: row n when it was split (chunk_off null: the one cluster-wide row
// of nch1 chunks).  The candidates are the row's chunk lists part [chunk][k].
__global__ __launch_bounds__(256) void k_top_merge(const int64_t* __restrict__ chunk_off, int64_t nch1, int32_t k,
                                                    const u64* __restrict__ part,
                                                    const int32_t* __restrict__ part_nz,
                                                    int32_t* __restrict__ out_rule, int32_t* __restrict__ out_cnt,
                                                    int32_t* __restrict__ out_nl, int32_t* __restrict__ out_nc) {
  __shared__ u64 sh_key[4][64];
  __shared__ int32_t sh_nz[4];
  const int64_t n = blockIdx.x;
  const int64_t c0 = chunk_off ? chunk_off[n] : 0, c1 = chunk_off ? chunk_off[n + 1] : nch1;
  if (c1 - c0 <= 1) return;  // the whole block: finished by k_top_select
  const int32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64* src = part + c0 * k;
  const int64_t total = (c1 - c0) * k;
  u64 held = 0, thr = 0;
  for (int64_t i0 = int64_t(wv) * 64; i0 < total; i0 += 256) {
    const int64_t i = i0 + lane;
    top_insert(i < total ? src[i] : 0, held, thr, k, lane);
  }
  int32_t nz = 0;
  for (int64_t c = c0 + threadIdx.x; c < c1; c += 256) nz += part_nz[c];
  nz = wave_sum(nz);
  sh_key[wv][lane] = held;
  if (lane == 0) sh_nz[wv] = nz;
  __syncthreads();
  if (wv != 0) return;
  for (int w = 1; w < 4; w++) top_insert(sh_key[w][lane], held, thr, k, lane);
  top_store_row(n, held, sh_nz[0] + sh_nz[1] + sh_nz[2] + sh_nz[3], k, lane, out_rule, out_cnt, out_nl, out_nc);
}

// ------------------------------------------------------------------ host --
int top_pending(cg_ctx* c) {
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  if (async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined rule-major calls pending (call cg_expand_wait first)");
  return CG_OK;
}

int top_check_k(const char* who, int32_t k) {
  if (k < 1 || k > CG_TOP_RULES_MAX)
    return cg_fail(CG_EINVAL, std::string(who) + ": k outside [1, " + std::to_string(CG_TOP_RULES_MAX) + "]");
  return CG_OK;
}

int top_no_profile() {
  return cg_fail(CG_EINVAL, "no profile result (the last profile call failed, or none was made)");
}

// The select and merge over `rows` rows cut into at most chunks_max chunks,
// c->tr_bucket [rows] already enqueued; nodes: the rows are the nodes of the
// profile's transpose, else the one row of all rules.  c->mu held, arguments
// checked; ends in a stream synchronise.
int top_run(cg_ctx* c, int32_t rows, int32_t k, bool nodes, int64_t chunks_max) {
  hipStream_t st = c->st;
  int rc;
  for (hipEvent_t& e : c->trev)
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  const size_t cells = size_t(std::max<int64_t>(int64_t(rows) * k, 1)), nr = size_t(std::max(rows, 1));
  if ((rc = c->tr_rule.ensure(cells)) || (rc = c->tr_cnt.ensure(cells)) || (rc = c->tr_nlisted.ensure(nr)) ||
      (rc = c->tr_ncontrib.ensure(nr)) || (rc = c->tr_part.ensure(size_t(chunks_max) * k)) ||
      (rc = c->tr_part_nz.ensure(size_t(chunks_max))))
    return rc;
  int64_t chunks = rows ? chunks_max : 0;  // of the nodes: read back below
  (void)hipEventRecord(c->trev[0], st);
  if (rows > 0) {
    const int64_t* off = nodes ? c->pf_chunk_off.p : nullptr;
    hipLaunchKernelGGL(k_top_select, dim3(unsigned((chunks_max + 3) / 4)), dim3(256), 0, st,
                       nodes ? c->nt_off.p : nullptr, nodes ? c->nt_rule.p : nullptr, off, rows, c->pf_R,
                       c->pf_rules.p, c->pf_B, c->tr_bucket.p, k, c->tr_rule.p, c->tr_cnt.p, c->tr_nlisted.p,
                       c->tr_ncontrib.p, c->tr_part.p, c->tr_part_nz.p);
    (void)hipEventRecord(c->trev[1], st);
    if (chunks_max > rows)
      hipLaunchKernelGGL(k_top_merge, dim3(unsigned(rows)), dim3(256), 0, st, off, chunks_max, k, c->tr_part.p,
                         c->tr_part_nz.p, c->tr_rule.p, c->tr_cnt.p, c->tr_nlisted.p, c->tr_ncontrib.p);
    (void)hipEventRecord(c->trev[2], st);
    HIPCHK(hipGetLastError());
    if (nodes) HIPCHK(hipMemcpyAsync(&chunks, c->pf_chunk_off.p + rows, 8, hipMemcpyDeviceToHost, st));
  } else {
    (void)hipEventRecord(c->trev[1], st);
    (void)hipEventRecord(c->trev[2], st);
  }
  HIPCHK(hipStreamSynchronize(st));
  (void)hipEventElapsedTime(&c->tr_ms[0], c->trev[0], c->trev[1]);
  (void)hipEventElapsedTime(&c->tr_ms[1], c->trev[1], c->trev[2]);
  if (chunks <= rows) c->tr_ms[1] = 0.f;  // no row was split
  c->tr_ms[2] = float(chunks);
  c->tr_rows = rows;
  c->tr_k = k;
  c->tr_valid = true;
  return CG_OK;
}

int top_no_result(const char* who) {
  return cg_fail(CG_EINVAL, std::string(who) + ": no top-rules result since the last profile call");
}

}  // namespace

extern "C" {

int cg_profile_top_rules_nodes(cg_ctx* c, int32_t k, const int32_t* bucket) {
  if (!c) return cg_fail(CG_EINVAL, "cg_profile_top_rules_nodes: null");
  if (int rc = top_check_k("cg_profile_top_rules_nodes", k)) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return top_no_profile();
  if (!c->pf_has_nodes) return cg_fail(CG_EINVAL, "the last profile has no node matrix (no per-node call)");
  if (c->pf_nt_gen != c->nt_gen)
    return cg_fail(CG_EINVAL,
                   "cg_profile_top_rules_nodes: the join the profile was built with has been replaced (a per-node "
                   "call with another rule set or exclude mode, or a dispatcher bind); repeat the profile call");
  const int32_t N = c->pf_N, B = c->pf_B;
  if (bucket)
    for (int32_t n = 0; n < N; n++)
      if (bucket[n] < 0 || bucket[n] >= B)
        return cg_fail(CG_EINVAL, "cg_profile_top_rules_nodes: node " + std::to_string(n) + ": bucket " +
                                      std::to_string(bucket[n]) + " outside [0, " + std::to_string(B) + ")");
  if (int rc = top_pending(c)) return rc;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  c->tr_valid = false;
  int rc;
  if ((rc = c->tr_bucket.ensure(size_t(std::max(N, 1))))) return rc;
  if (N > 0) {
    if (bucket) {
      // (the caller's array outlives the stream synchronise that ends the call)
      HIPCHK(hipMemcpyAsync(c->tr_bucket.p, bucket, size_t(N) * 4, hipMemcpyHostToDevice, c->st));
    } else {
      if (!c->pf_peaks_valid) {
        if ((rc = c->pf_peak.ensure(size_t(N))) || (rc = c->pf_peak_bucket.ensure(size_t(N)))) return rc;
        if ((rc = profile_node_peaks_enqueue(c))) return rc;
      }
      HIPCHK(hipMemcpyAsync(c->tr_bucket.p, c->pf_peak_bucket.p, size_t(N) * 4, hipMemcpyDeviceToDevice, c->st));
    }
  }
  // as the node matrix: at most one chunk per node plus one per kNodeChunk pairs
  if ((rc = top_run(c, N, k, true, int64_t(N) + c->pf_nnz / kNodeChunk + 1))) return rc;
  if (!bucket && N > 0) c->pf_peaks_valid = true;  // the stream has drained: the peaks are there
  return CG_OK;
}

int cg_profile_top_rules_bucket(cg_ctx* c, int32_t bucket, int32_t k) {
  if (!c) return cg_fail(CG_EINVAL, "cg_profile_top_rules_bucket: null");
  if (int rc = top_check_k("cg_profile_top_rules_bucket", k)) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pf_valid) return top_no_profile();
  if (bucket < 0 || bucket >= c->pf_B)
    return cg_fail(CG_EINVAL, "cg_profile_top_rules_bucket: bucket " + std::to_string(bucket) + " outside [0, " +
                                  std::to_string(c->pf_B) + ")");
  if (int rc = top_pending(c)) return rc;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  c->tr_valid = false;
  int rc;
  if ((rc = c->tr_bucket.ensure(1))) return rc;
  HIPCHK(hipMemcpyAsync(c->tr_bucket.p, &bucket, 4, hipMemcpyHostToDevice, c->st));
  const int64_t R = c->pf_R;
  return top_run(c, 1, k, false, R <= kNodeChunk ? 1 : (R + kNodeChunk - 1) / kNodeChunk);
}

int cg_profile_top_rules_copy(cg_ctx* c, int32_t first, int32_t count, int32_t* rule, int32_t* cnt,
                              int32_t* n_listed, int32_t* n_contrib, int32_t* bucket) {
  if (!c) return cg_fail(CG_EINVAL, "cg_profile_top_rules_copy: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->tr_valid) return top_no_result("cg_profile_top_rules_copy");
  if (first < 0 || count < 0 || int64_t(first) + count > c->tr_rows)
    return cg_fail(CG_EINVAL, "cg_profile_top_rules_copy: row range outside the last top-rules result");
  if (!count) return CG_OK;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  const size_t k = size_t(c->tr_k), n = size_t(count), f = size_t(first);
  hipStream_t st = c->st;
  if (rule) HIPCHK(hipMemcpyAsync(rule, c->tr_rule.p + f * k, n * k * 4, hipMemcpyDeviceToHost, st));
  if (cnt) HIPCHK(hipMemcpyAsync(cnt, c->tr_cnt.p + f * k, n * k * 4, hipMemcpyDeviceToHost, st));
  if (n_listed) HIPCHK(hipMemcpyAsync(n_listed, c->tr_nlisted.p + f, n * 4, hipMemcpyDeviceToHost, st));
  if (n_contrib) HIPCHK(hipMemcpyAsync(n_contrib, c->tr_ncontrib.p + f, n * 4, hipMemcpyDeviceToHost, st));
  if (bucket) HIPCHK(hipMemcpyAsync(bucket, c->tr_bucket.p + f, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return CG_OK;
}

int cg_profile_top_rules_device(cg_ctx* c, const int32_t** d_rule, const int32_t** d_cnt,
                                const int32_t** d_n_listed, const int32_t** d_n_contrib, const int32_t** d_bucket,
                                int32_t* rows, int32_t* k) {
  if (!c) return cg_fail(CG_EINVAL, "cg_profile_top_rules_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->tr_valid) return top_no_result("cg_profile_top_rules_device");
  if (d_rule) *d_rule = c->tr_rule.p;
  if (d_cnt) *d_cnt = c->tr_cnt.p;
  if (d_n_listed) *d_n_listed = c->tr_nlisted.p;
  if (d_n_contrib) *d_n_contrib = c->tr_ncontrib.p;
  if (d_bucket) *d_bucket = c->tr_bucket.p;
  if (rows) *rows = c->tr_rows;
  if (k) *k = c->tr_k;
  return CG_OK;
}

int cg_profile_top_rules_times(cg_ctx* c, float* ms, int n) {
  if (!c || !ms || n < 0) return cg_fail(CG_EINVAL, "cg_profile_top_rules_times: null");
  std::lock_guard<std::mutex> g(c->mu);
  const int m = std::min(n, 3);
  for (int i = 0; i < m; i++) ms[i] = c->tr_ms[i];
  return m;
}

}  // extern "C"
