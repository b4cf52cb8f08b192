// cg_rule_nodes.hip -- rule -> node resolution (CSR join) on gfx950 and its
// node-major transpose, for the per-node lists (cg_pernode.hip) and the
// dispatcher's fan-out (cg_fanout.hip).
//
// Reference semantics (job.go:274-288, 591-630; group.go:111-119;
// web/job.go:222-257): a rule runs on node n when n is one of its NodeIDs or a
// member of one of its (existing) GroupIDs, the job is not paused, and --
// depending on the exclude mode -- n is not excluded.  Every cronsun node
// evaluates this for itself over all jobs (node/node.go:121-158); here one
// pass builds the whole rule -> node CSR.
//
// Pipeline:
//   k_rule_nodes<false>  one wave per rule: node bitmap in LDS (ds_or), count
//   scan                 -> rule->node CSR offsets
//   k_rule_nodes<true>   same bitmap, ballot/prefix-sum compaction of set bits
//   k_rs_hist/scatter    stable LSD radix transpose to node -> rules (8 bits a pass)
//   k_node_bounds        per-node pair offsets (lower bound per node)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_kernels.h"

using namespace cg;

namespace {

struct RulesDev {
  const int64_t* nid_off;
  const int32_t* nids;
  const int64_t* gid_off;
  const int32_t* gids;
  const int64_t* ex_off;
  const int32_t* ex;
  const int32_t* rule_job;
  const uint8_t* job_pause;
  const int64_t* group_off;
  const int32_t* group_nodes;
  const uint8_t* group_exists;
  const int32_t* next_same;  // next rule of the job with the same Cmd key, -1; null: none repeats
  const int32_t* prev_same;  // the previous one, -1 (with next_same)
  int32_t R, G, N, words;
};

// wave-local LDS hand-off (the rules of HIP's __syncwarp: release fence,
// wave barrier, acquire fence)
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void bm_set(uint32_t* bm, int32_t n, int32_t N) {
  if (n >= 0 && n < N) atomicOr(&bm[n >> 5], 1u << (n & 31));
}
__device__ __forceinline__ void bm_clear(uint32_t* bm, int32_t n, int32_t N) {
  if (n >= 0 && n < N) atomicAnd(&bm[n >> 5], ~(1u << (n & 31)));
}

// Rule q's node set under `mode` into the wave's bitmap bm (zeroed here):
// NodeIDs and existing groups' members (JobRule.included job.go:274-288,
// Group.Included group.go:111-119), minus the mode's excludes; empty for a
// paused job (job.go:593).
__device__ void rule_bitmap(const RulesDev& d, int mode, int64_t q, uint32_t* bm, int lane) {
  for (int w = lane; w < d.words; w += 64) bm[w] = 0;
  wave_sync_lds();
  const int32_t job = d.rule_job[q];
  if (d.job_pause[job]) return;
  for (int64_t k = d.nid_off[q] + lane; k < d.nid_off[q + 1]; k += 64) bm_set(bm, d.nids[k], d.N);
  for (int64_t k = d.gid_off[q]; k < d.gid_off[q + 1]; k++) {
    int32_t g = d.gids[k];
    if (g < 0 || g >= d.G || !d.group_exists[g]) continue;  // gs[gid] missing
    for (int64_t p = d.group_off[g] + lane; p < d.group_off[g + 1]; p += 64)
      bm_set(bm, d.group_nodes[p], d.N);
  }
  wave_sync_lds();
  if (mode == CG_EXCLUDE_RULE) {
    for (int64_t k = d.ex_off[q] + lane; k < d.ex_off[q + 1]; k += 64) bm_clear(bm, d.ex[k], d.N);
  } else if (mode == CG_EXCLUDE_CUMULATIVE) {
    int64_t r0 = q;
    while (r0 > 0 && d.rule_job[r0 - 1] == job) r0--;
    for (int64_t p = r0; p <= q; p++)
      for (int64_t k = d.ex_off[p] + lane; k < d.ex_off[p + 1]; k += 64) bm_clear(bm, d.ex[k], d.N);
  }
  wave_sync_lds();
}

// One wave per rule r: r's node set (rule_bitmap) minus the node sets of the
// later rules of r's job with the same Cmd key -- Job.Cmds' map keeps the
// last included rule per Job.ID+Rule.ID (job.go:604-609) -- then either the
// count (WRITE false) or the ballot/prefix compaction of the set bits into the
// rule-major pairs (WRITE true).  With repeated keys the wave of a key's last
// rule sweeps the key's rules from last to first, keeping the union of the
// later ones' sets in a second bitmap (sh): every rule's set is built once
// (a job with k rules of one key costs k bitmap builds, not k^2 / 2); the
// other rules' waves have nothing to do.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_rule_nodes(RulesDev d, int mode, int wpb,
                                                     int32_t* __restrict__ rn_cnt,
                                                     const int64_t* __restrict__ rn_off,
                                                     int32_t* __restrict__ rn_nodes,
                                                     int32_t* __restrict__ pair_rule) {
  extern __shared__ uint32_t bm_all[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave >= wpb) return;
  const bool dup = d.next_same != nullptr;
  uint32_t* bm = bm_all + size_t(wave) * (dup ? 2 : 1) * d.words;
  uint32_t* sh = bm + d.words;  // dup: union of the later same-key rules' sets
  for (int64_t r = int64_t(blockIdx.x) * wpb + wave; r < d.R; r += int64_t(gridDim.x) * wpb) {
    if (dup) {
      if (d.next_same[r] >= 0) continue;  // the key's last rule sweeps it
      for (int w = lane; w < d.words; w += 64) sh[w] = 0;
    }
    int64_t q = r;
    do {
      rule_bitmap(d, mode, q, bm, lane);
      if (!WRITE) {
        int32_t c = 0;
        for (int w = lane; w < d.words; w += 64) c += __popc(dup ? bm[w] & ~sh[w] : bm[w]);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) rn_cnt[q] = c;
      } else {
        int64_t pos = rn_off[q];
        for (int base = 0; base < d.words; base += 64) {
          int w = base + lane;
          uint32_t bits = w < d.words ? (dup ? bm[w] & ~sh[w] : bm[w]) : 0u;
          int32_t c = __popc(bits);
          int32_t inc = c;
          for (int o = 1; o < 64; o <<= 1) {
            int32_t y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
          }
          int64_t p = pos + inc - c;
          while (bits) {
            int b = __builtin_ctz(bits);
            bits &= bits - 1;
            rn_nodes[p] = w * 32 + b;
            pair_rule[p] = int32_t(q);
            p++;
          }
          pos += __shfl(inc, 63, 64);
        }
      }
      if (!dup) break;
      q = d.prev_same[q];
      if (q >= 0)
        for (int w = lane; w < d.words; w += 64) sh[w] |= bm[w];
      wave_sync_lds();
    } while (q >= 0);
    wave_sync_lds();
  }
}

// nt_off[n] = first position of node n in the node-sorted pairs (n <= N):
// a lower bound per node, no atomics (a histogram of sorted keys would put
// every lane of a wave on the same counter)
__global__ void k_node_bounds(const uint32_t* __restrict__ keys, int64_t n, int32_t N,
                              int64_t* __restrict__ nt_off) {
  const int64_t v = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (v > N) return;
  int64_t lo = 0, hi = n;  // first index with keys[i] >= v
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (int64_t(keys[mid]) < v) lo = mid + 1;
    else hi = mid;
  }
  nt_off[v] = lo;
}

// ---- transpose: stable LSD radix sort of the rule-major (node, rule) pairs
// by node, 8 bits per pass.  Each pass keeps the order of equal digits, so
// rules stay ascending within every node (the order Job.Cmds is evaluated in
// when a node walks the jobs, job.go:591-614). ----
constexpr int kRsItems = 16;
constexpr int kRsTile = 256 * kRsItems;  // pairs per block
constexpr int kRsBuckets = 256;

__global__ __launch_bounds__(256) void k_rs_hist(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                  int32_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t h[kRsBuckets];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = int64_t(blockIdx.x) * kRsTile;
  for (int j = 0; j < kRsItems; j++) {
    const int64_t i = base + j * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & (kRsBuckets - 1)], 1u);
  }
  __syncthreads();
  hist[int64_t(threadIdx.x) * nb + blockIdx.x] = int32_t(h[threadIdx.x]);  // digit-major
}

// One pass's stable scatter.  Input order inside a block: wave w owns pairs
// [tile + w*1024, +1024), item j the 64 pairs [j*64, j*64 + 64) of those.  A
// pair's rank among equal digits = earlier items of its wave (running counts
// in LDS) + earlier lanes of its item (8-ballot multisplit) + earlier waves
// (prefix per digit) + earlier blocks (the scanned digit-major histogram).
__global__ __launch_bounds__(256) void k_rs_scatter(const uint32_t* __restrict__ kin,
                                                     const int32_t* __restrict__ vin, int64_t n, int shift,
                                                     const int64_t* __restrict__ off, int64_t nb,
                                                     uint32_t* __restrict__ kout, int32_t* __restrict__ vout) {
  __shared__ int32_t run[4][kRsBuckets];
  __shared__ int64_t base_of[4][kRsBuckets];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * kRsBuckets; i += 256) (&run[0][0])[i] = 0;
  __syncthreads();
  const int64_t base = int64_t(blockIdx.x) * kRsTile + int64_t(w) * (64 * kRsItems);
  const uint64_t lt = (1ull << lane) - 1ull;
  uint32_t key[kRsItems];
  int32_t val[kRsItems], rk[kRsItems];
#pragma unroll
  for (int j = 0; j < kRsItems; j++) {
    const int64_t i = base + j * 64 + lane;
    key[j] = i < n ? kin[i] : 0u;
    val[j] = i < n ? vin[i] : 0;
  }
#pragma unroll
  for (int j = 0; j < kRsItems; j++) {
    const bool valid = base + j * 64 + lane < n;
    const uint32_t d = (key[j] >> shift) & (kRsBuckets - 1);
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    // every lane reads the running count before the group's first lane adds
    // the group size (a wave's LDS operations complete in program order)
    const int32_t r0 = run[w][d];
    rk[j] = r0 + __popcll(peers & lt);
    if (valid && (peers & lt) == 0) run[w][d] = r0 + __popcll(peers);
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    int64_t acc = off[int64_t(d) * nb + blockIdx.x];
    for (int ww = 0; ww < 4; ww++) {
      base_of[ww][d] = acc;
      acc += run[ww][d];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRsItems; j++) {
    if (base + j * 64 + lane >= n) continue;
    const int64_t pos = base_of[w][(key[j] >> shift) & (kRsBuckets - 1)] + rk[j];
    kout[pos] = key[j];
    vout[pos] = val[j];
  }
}

template <class T>
int upload(DBuf<T>& b, const T* h, size_t n, hipStream_t st) {
  int rc = b.ensure(std::max<size_t>(n, 1));
  if (rc) return rc;
  if (n) return cg_hip_check(hipMemcpyAsync(b.p, h, n * sizeof(T), hipMemcpyHostToDevice, st),
                             "hipMemcpyAsync(rules)");
  return CG_OK;
}

int validate_rules(const cg_rules_in* in) {
  if (in->n_rules < 0 || in->n_nodes < 0 || in->n_groups < 0 || in->n_jobs < 0)
    return cg_fail(CG_EINVAL, "negative sizes");
  if (in->n_rules && (!in->nid_off || !in->gid_off || !in->ex_off || !in->rule_job))
    return cg_fail(CG_EINVAL, "rules arrays missing");
  if (in->n_groups && (!in->group_off || !in->group_exists))
    return cg_fail(CG_EINVAL, "group arrays missing");
  if (in->n_jobs && !in->job_pause) return cg_fail(CG_EINVAL, "job_pause missing");
  std::vector<uint8_t> seen(size_t(std::max(in->n_jobs, 1)), 0);
  for (int32_t r = 0; r < in->n_rules; r++) {
    int32_t j = in->rule_job[r];
    if (j < 0 || j >= in->n_jobs) return cg_fail(CG_EINVAL, "rule_job out of range");
    if (r == 0 || j != in->rule_job[r - 1]) {
      if (seen[j]) return cg_fail(CG_EINVAL, "a job's rules must be contiguous");
      seen[j] = 1;
    }
  }
  auto check_list = [&](const int64_t* off, const int32_t* v, int64_t cnt, int64_t lim,
                        const char* what) -> int {
    if (off[0] != 0) return cg_fail(CG_EINVAL, std::string(what) + ": offsets must start at 0");
    for (int64_t i = 0; i < cnt; i++)
      if (off[i + 1] < off[i]) return cg_fail(CG_EINVAL, std::string(what) + ": offsets decrease");
    for (int64_t k = 0; k < off[cnt]; k++)
      if (v[k] < 0 || v[k] >= lim) return cg_fail(CG_EINVAL, std::string(what) + ": index out of range");
    return CG_OK;
  };
  int rc;
  if (in->n_rules) {
    if ((rc = check_list(in->nid_off, in->nids, in->n_rules, in->n_nodes, "nids"))) return rc;
    if ((rc = check_list(in->gid_off, in->gids, in->n_rules, in->n_groups, "gids"))) return rc;
    // an ExcludeNodeID may name a node the cluster no longer has: any id >= 0
    if ((rc = check_list(in->ex_off, in->ex, in->n_rules, int64_t(INT32_MAX) + 1, "exclude_nids"))) return rc;
  }
  if (in->n_groups && (rc = check_list(in->group_off, in->group_nodes, in->n_groups, in->n_nodes, "groups")))
    return rc;
  return CG_OK;
}

}  // namespace

// validates a host rule set and copies it into a device store
int upload_rules(const cg_rules_in* in, RulesStore* st, hipStream_t s) {
  int rc = validate_rules(in);
  if (rc) return rc;
  const int32_t R = in->n_rules, G = in->n_groups;
  const int64_t n_nid = R ? in->nid_off[R] : 0, n_gid = R ? in->gid_off[R] : 0,
                n_ex = R ? in->ex_off[R] : 0, n_gn = G ? in->group_off[G] : 0;
  if ((rc = upload(st->nid_off, in->nid_off, R ? R + 1 : 0, s))) return rc;
  if ((rc = upload(st->nids, in->nids, n_nid, s))) return rc;
  if ((rc = upload(st->gid_off, in->gid_off, R ? R + 1 : 0, s))) return rc;
  if ((rc = upload(st->gids, in->gids, n_gid, s))) return rc;
  if ((rc = upload(st->ex_off, in->ex_off, R ? R + 1 : 0, s))) return rc;
  if ((rc = upload(st->ex, in->ex, n_ex, s))) return rc;
  if ((rc = upload(st->rule_job, in->rule_job, R, s))) return rc;
  if ((rc = upload(st->job_pause, in->job_pause, in->n_jobs, s))) return rc;
  if ((rc = upload(st->group_off, in->group_off, G ? G + 1 : 0, s))) return rc;
  if ((rc = upload(st->group_nodes, in->group_nodes, n_gn, s))) return rc;
  if ((rc = upload(st->group_exists, in->group_exists, G, s))) return rc;
  // Cmd keys: next_same[r] = the next rule of r's job with r's key (Job.Cmds'
  // later-rule-wins map, job.go:604-609), uploaded only when a key repeats
  std::vector<int32_t> next_same, prev_same;
  st->has_dup = false;
  if (in->rule_key && R) {
    next_same.assign(size_t(R), -1);
    prev_same.assign(size_t(R), -1);
    std::unordered_map<int32_t, int32_t> last;  // key -> the job's latest rule seen (walking back)
    for (int32_t r = R - 1; r >= 0; r--) {
      if (r == R - 1 || in->rule_job[r] != in->rule_job[r + 1]) last.clear();
      auto it = last.find(in->rule_key[r]);
      if (it != last.end()) {
        next_same[size_t(r)] = it->second;
        prev_same[size_t(it->second)] = r;
        it->second = r;
        st->has_dup = true;
      } else {
        last.emplace(in->rule_key[r], r);
      }
    }
  }
  if (st->has_dup && ((rc = upload(st->next_same, next_same.data(), size_t(R), s)) ||
                      (rc = upload(st->prev_same, prev_same.data(), size_t(R), s))))
    return rc;
  st->n_nodes = in->n_nodes;
  st->n_groups = G;
  st->n_rules = R;
  st->n_jobs = in->n_jobs;
  static std::atomic<uint64_t> next_serial{1};
  st->serial = next_serial.fetch_add(1);
  return cg_hip_check(hipStreamSynchronize(s), "upload rules");  // host arrays may go away
}

// builds the rule->node CSR on the device; leaves rn_off/rn_nodes/pair_rule in ctx
int rule_nodes_locked(cg_ctx* c, const RulesStore& st, int mode, int64_t* nnz_out) {
  if (mode < 0 || mode > 2) return cg_fail(CG_EINVAL, "bad exclude mode");
  const int32_t R = st.n_rules, G = st.n_groups, N = st.n_nodes;
  const int32_t words = (N + 31) / 32;
  if (size_t(words) * 4 * (st.has_dup ? 2 : 1) > 64 * 1024)
    return cg_fail(CG_ERANGE, st.has_dup ? "more than 262144 nodes with repeated Cmd keys"
                                         : "more than 524288 nodes");
  hipStream_t s = c->st;
  int rc;
  if ((rc = c->rn_cnt.ensure(std::max(R, 1)))) return rc;
  if ((rc = c->rn_off.ensure(R + 1))) return rc;
  if ((rc = c->scan_tmp.ensure(std::max(c->scan_tmp.cap, scan_temp_bytes(R))))) return rc;
  RulesDev d{st.nid_off.p, st.nids.p, st.gid_off.p, st.gids.p, st.ex_off.p, st.ex.p,
             st.rule_job.p, st.job_pause.p, st.group_off.p, st.group_nodes.p,
             st.group_exists.p, st.has_dup ? st.next_same.p : nullptr,
             st.has_dup ? st.prev_same.p : nullptr, R, G, N, std::max(words, 1)};
  const size_t per = st.has_dup ? 2 : 1;  // a second bitmap per wave for repeated Cmd keys
  int wpb = int(std::min<size_t>(4, std::max<size_t>(1, (64 * 1024) / (per * size_t(d.words) * 4))));
  size_t lds = size_t(wpb) * per * d.words * 4;
  int grid = gridn(R, wpb, 256 * 16);
  if (R > 0)
    hipLaunchKernelGGL(k_rule_nodes<false>, dim3(grid), dim3(64 * wpb), lds, s, d, mode, wpb,
                       c->rn_cnt.p, nullptr, nullptr, nullptr);
  launch_scan(c->rn_cnt.p, c->rn_off.p, R, c->scan_tmp.p, s);
  int64_t nnz = 0;
  if ((rc = cg_hip_check(hipMemcpyAsync(&nnz, c->rn_off.p + R, 8, hipMemcpyDeviceToHost, s), "nnz")))
    return rc;
  if ((rc = cg_hip_check(hipStreamSynchronize(s), "sync"))) return rc;
  if ((rc = c->rn_nodes.ensure(std::max<int64_t>(nnz, 1)))) return rc;
  if ((rc = c->pair_rule.ensure(std::max<int64_t>(nnz, 1)))) return rc;
  if (R > 0 && nnz > 0)
    hipLaunchKernelGGL(k_rule_nodes<true>, dim3(grid), dim3(64 * wpb), lds, s, d, mode, wpb,
                       nullptr, c->rn_off.p, c->rn_nodes.p, c->pair_rule.p);
  if ((rc = cg_hip_check(hipGetLastError(), "k_rule_nodes"))) return rc;
  *nnz_out = nnz;
  return CG_OK;
}

int64_t radix_hist_words(int64_t n) { return kRsBuckets * ((n + kRsTile - 1) / kRsTile); }

void radix_by_key_enqueue(hipStream_t st, uint32_t* k0, int32_t* v0, uint32_t* k1, int32_t* v1, int64_t n,
                          int32_t N, int32_t* hist, int64_t* off, void* scan_tmp, bool* in_second) {
  *in_second = false;
  if (n <= 0) return;
  const int64_t nb = (n + kRsTile - 1) / kRsTile;
  uint32_t *kin = k0, *kout = k1;
  int32_t *vin = v0, *vout = v1;
  for (int shift = 0; shift == 0 || (int64_t(1) << shift) < int64_t(N); shift += 8) {
    hipLaunchKernelGGL(k_rs_hist, dim3(unsigned(nb)), dim3(256), 0, st, kin, n, shift, hist, nb);
    launch_scan(hist, off, kRsBuckets * nb, scan_tmp, st);
    hipLaunchKernelGGL(k_rs_scatter, dim3(unsigned(nb)), dim3(256), 0, st, kin, vin, n, shift, off, nb, kout,
                       vout);
    std::swap(kin, kout);
    std::swap(vin, vout);
    *in_second = !*in_second;
  }
}

void launch_node_bounds(hipStream_t st, const uint32_t* keys, int64_t n, int32_t N, int64_t* off) {
  hipLaunchKernelGGL(k_node_bounds, dim3(gridn(int64_t(N) + 1, 256, 1 << 30)), dim3(256), 0, st, keys, n, N, off);
}

// Stable transpose of the rule-major pairs (rn_nodes, pair_rule) into node
// order: nt_rule (rules ascending within a node) and nt_off[N+1].
int transpose_locked(cg_ctx* c, int64_t nnz, int32_t N) {
  hipStream_t st = c->st;
  int rc;
  c->nt_gen++;  // whatever was built from the old lists no longer matches them
  if ((rc = c->nt_rule.ensure(std::max<int64_t>(nnz, 1)))) return rc;
  if ((rc = c->pair_node.ensure(std::max<int64_t>(nnz, 1)))) return rc;
  if ((rc = c->nt_off.ensure(N + 1))) return rc;
  if (nnz > 0) {
    const int64_t hw = radix_hist_words(nnz);
    if ((rc = c->rs_hist.ensure(hw))) return rc;
    if ((rc = c->rs_off.ensure(hw + 1))) return rc;
    if ((rc = c->scan_tmp.ensure(std::max(c->scan_tmp.cap, scan_temp_bytes(hw))))) return rc;
    bool in_second = false;
    radix_by_key_enqueue(st, reinterpret_cast<uint32_t*>(c->rn_nodes.p), c->pair_rule.p,
                         reinterpret_cast<uint32_t*>(c->pair_node.p), c->nt_rule.p, nnz, N, c->rs_hist.p,
                         c->rs_off.p, c->scan_tmp.p, &in_second);
    // keep the sorted pairs in (pair_node, nt_rule)
    if (!in_second) {
      std::swap(c->rn_nodes, c->pair_node);
      std::swap(c->pair_rule, c->nt_rule);
    }
  }
  launch_node_bounds(st, reinterpret_cast<const uint32_t*>(c->pair_node.p), nnz, N, c->nt_off.p);
  return cg_hip_check(hipGetLastError(), "transpose");
}

extern "C" {

int cg_rule_nodes(cg_ctx* c, const cg_rules_in* in, int mode, int64_t* rn_off, int32_t* rn_nodes,
                  int64_t cap, int64_t* nnz) {
  if (!c || !in || !nnz) return cg_fail(CG_EINVAL, "cg_rule_nodes: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  if ((rc = upload_rules(in, &c->rules, c->st))) return rc;
  if ((rc = rule_nodes_locked(c, c->rules, mode, nnz))) return rc;
  if ((rc = cg_hip_check(hipStreamSynchronize(c->st), "sync"))) return rc;
  if (rn_off &&
      (rc = cg_hip_check(hipMemcpy(rn_off, c->rn_off.p, size_t(in->n_rules + 1) * 8, hipMemcpyDeviceToHost),
                         "copy rn_off")))
    return rc;
  if (rn_nodes) {
    if (cap < *nnz) return cg_fail(CG_ECAPACITY, "rn_nodes buffer too small; see nnz");
    if (*nnz && (rc = cg_hip_check(hipMemcpy(rn_nodes, c->rn_nodes.p, size_t(*nnz) * 4, hipMemcpyDeviceToHost),
                                   "copy rn_nodes")))
      return rc;
  }
  return CG_OK;
}

int cg_rules_upload(cg_ctx* c, const cg_rules_in* in, cg_rules** out) {
  if (!c || !in || !out) return cg_fail(CG_EINVAL, "cg_rules_upload: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  cg_rules* r = new cg_rules();
  r->ctx = c;
  if ((rc = upload_rules(in, &r->st, c->st))) {
    r->st.release();
    delete r;
    return rc;
  }
  *out = r;
  return CG_OK;
}

void cg_rules_free(cg_rules* r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  r->st.release();
  delete r;
}

}  // extern "C"
