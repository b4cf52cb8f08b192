// cg_pernode.hip -- per-node fire lists on gfx950: every node's copy of the
// fire times of the rules that run on it (the rule -> node join and its
// transpose: cg_rule_nodes.hip), through the synchronous and the pipelined
// entry points and the result accessors.
//
// Pipeline, per window over the cached node-major pairs:
//   k_seg_bounds         (node, rule band) segment bounds (cached per band width)
//   k_rule_info          per rule: fire count, first fire, progression stride
//   k_seg_records -> scan  per segment: events, compact pair records -> offsets
//   k_node_write         per segment, in band- or node-major order: each node's
//                        copy of its rules' fire times (whole 64-event blocks;
//                        pairs placed by a wave prefix sum, blocks spanning pairs
//                        resolved by an LDS start mask + popcount)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/cronsun_gpu.h"
#include "cg_api_internal.h"
#include "cg_kernels.h"

using namespace cg;

namespace {

// ---- per-call segments: (node n, rule band k) = node n's pairs whose rule is
// in [k*B, (k+1)*B).  Bands keep a band's rule fire lists (and their
// offsets) L2-resident while every node's segment of the band is written. ----

// seg_pair[n*K + k] = first pair of node n with rule >= k*B; [N*K] = nnz
__global__ void k_seg_bounds(const int64_t* __restrict__ nt_off, const int32_t* __restrict__ nt_rule,
                             int32_t N, int32_t K, int32_t B, int64_t* __restrict__ seg_pair) {
  const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  const int64_t NK = int64_t(N) * K;
  if (t > NK) return;
  if (t == NK) {
    seg_pair[t] = nt_off[N];
    return;
  }
  const int32_t n = int32_t(t / K), k = int32_t(t - int64_t(n) * K);
  int64_t lo = nt_off[n], hi = nt_off[n + 1];
  const int64_t x = int64_t(k) * B;
  while (lo < hi) {  // first pair with rule >= x
    const int64_t mid = (lo + hi) >> 1;
    if (int64_t(nt_rule[mid]) < x) lo = mid + 1;
    else hi = mid;
  }
  seg_pair[t] = lo;
}

// Per rule of the window's rule-major CSR, one 16-byte RuleInfo: its fire
// count, the band-relative index of its first fire, and whether its fires
// form an arithmetic progression {first fire - t0, stride} (stride 0: they do
// not, or it does not fit 32 bits).  In a 1-h window nearly every rule's
// fires are one (`0 */5 * * * *`, `@every`, `*/10 * * * * *`, any rule with
// <= 2 fires: 95 % of config 3's events), and the per-node writer computes
// those fires instead of gathering them.  k_seg_records then reads one
// 16-byte word per pair instead of three scattered ones.  One block per 256
// rules: lanes take the block's events in turn, find their rule by a binary
// search over the block's offsets in LDS and clear the rule's flag on a step
// that differs from its first one.
#ifndef CG_NODE_AP
#define CG_NODE_AP 1
#endif
constexpr int kApRules = 256;
inline int64_t rule_info_slots(int64_t R) { return std::max<int64_t>(R, 1); }
__global__ __launch_bounds__(256) void k_rule_info(const int64_t* __restrict__ rule_off,
                                                    const int64_t* __restrict__ times, int64_t R, int64_t t0,
                                                    int32_t B, int64_t cap, RuleInfo* __restrict__ info,
                                                    int64_t* __restrict__ err) {
  __shared__ int64_t off[kApRules + 1];
  __shared__ int64_t step[kApRules];
  __shared__ int32_t ok[kApRules];
  const int64_t r0 = int64_t(blockIdx.x) * kApRules;
  const int nr = int(R - r0 < kApRules ? R - r0 : kApRules);
  const int tid = threadIdx.x;
  if (rule_off[R] > cap) {  // a pipelined window past the fire-time capacity: no fires read, none written
    if (tid < nr) info[r0 + tid] = RuleInfo{0, 0, 0, 0};
    return;
  }
  const int64_t band_lo = rule_off[(r0 / B) * B];  // B is a multiple of kApRules
  // the writer's 32-bit band-relative indices and k_seg_records' int32
  // scans need a band to hold < 2^30 events (else the call fails)
  if (r0 % B == 0 && threadIdx.x == 0 && rule_off[r0 + B < R ? r0 + B : R] - band_lo > (int64_t(1) << 30))
    err[0] = 1;
  int64_t first = 0, cnt = 0;
  if (tid < nr) {
    const int64_t a = rule_off[r0 + tid];
    cnt = rule_off[r0 + tid + 1] - a;
    first = cnt > 0 ? times[a] : 0;
    off[tid] = a;
    step[tid] = cnt > 1 ? times[a + 1] - first : 1;
    ok[tid] = CG_NODE_AP;
  }
  if (tid == 0) off[nr] = rule_off[r0 + nr];
  __syncthreads();
  const int64_t e_end = off[nr];
  // kRiUnroll events per thread per round, their loads issued together: a
  // block whose rules fire thousands of times in the window (every-second
  // rules) walks a long span, and one dependent load pair per round made it
  // the kernel's latency tail
  constexpr int kRiUnroll = 4;
  for (int64_t e0 = off[0] + tid; e0 + 1 < e_end; e0 += int64_t(blockDim.x) * kRiUnroll) {
    int64_t ta[kRiUnroll], tb[kRiUnroll];
#pragma unroll
    for (int u = 0; u < kRiUnroll; u++) {
      const int64_t e = e0 + int64_t(u) * blockDim.x;
      const int64_t ec = e + 1 < e_end ? e : e_end - 2;  // clamped: every load in range
      ta[u] = times[ec];
      tb[u] = times[ec + 1];
    }
#pragma unroll
    for (int u = 0; u < kRiUnroll; u++) {
      const int64_t e = e0 + int64_t(u) * blockDim.x;
      if (e + 1 >= e_end) break;
      int lo = 0, hi = nr - 1;  // the last rule whose list starts at or before e
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
      }
      if (e + 1 < off[lo + 1] && tb[u] - ta[u] != step[lo]) ok[lo] = 0;
    }
  }
  __syncthreads();
  if (tid < nr) {
    const int64_t rel = first - t0, s = step[tid];
    const bool prog = cnt > 0 && ok[tid] && rel >= 0 && rel <= INT32_MAX && s > 0 && s <= INT32_MAX;
    // counts and band-relative indices are < 2^30 (k_seg_records checks the
    // band span and fails the call otherwise)
    info[r0 + tid] = RuleInfo{int32_t(cnt), int32_t(off[tid] - band_lo),
                              prog ? int32_t(rel) : 0, prog ? int32_t(s) : 0};
  }
}

// Inclusive scan of x within each 32-lane half of the wave, by DPP (no LDS
// round trips): row_shr 1/2/4/8 inside each 16-lane row, then row_bcast:15
// adds the last lane of rows 0 and 2 to rows 1 and 3.
__device__ __forceinline__ int32_t scan_halves(int32_t x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
  return x;
}
// lane 31's value in the low half, lane 63's in the high half
__device__ __forceinline__ int32_t half_total(int32_t incl) {
  const int32_t lo = __builtin_amdgcn_readlane(incl, 31), hi = __builtin_amdgcn_readlane(incl, 63);
  return (threadIdx.x & 63) < 32 ? lo : hi;
}

#ifndef CG_SEG_PAIRS_PER_LANE
#define CG_SEG_PAIRS_PER_LANE 8
#endif
constexpr int kSegPairsPerLane = CG_SEG_PAIRS_PER_LANE;
constexpr int kSegWavesPerSimd = 1;  // min waves per SIMD of k_seg_records (caps its VGPRs; 1: no cap)

// Segment records, one wave per segment in band-major order (a band's
// offsets stay in L2): the segment's event count, and for each of its
// non-empty pairs (in order, compacted to the front of the segment's pair
// range) a record {rule, first event relative to the segment, x, stride}:
// for a progression rule (k_rule_info) x = first fire - t0 - position * stride,
// so its fire at segment position p is t0 + x + p * stride; otherwise stride
// is 0 and x = band-relative fire-list index minus the position.  The writer
// then reads plain records instead of chasing pair -> rule -> offsets per
// window.  Block 0 also resets the writer's tickets; err[0] is set if a
// segment or a band outgrows the writer's 32-bit positions.
__global__ __launch_bounds__(256, kSegWavesPerSimd) void k_seg_records(const int64_t* __restrict__ seg_pair,
                                                      const int32_t* __restrict__ nt_rule,
                                                      const int64_t* __restrict__ rule_off,
                                                      const RuleInfo* __restrict__ info, int32_t N,
                                                      int32_t K, int32_t B, int64_t R,
                                                      int64_t* __restrict__ seg_cnt,
                                                      int32_t* __restrict__ seg_nrec,
                                                      PairRec* __restrict__ recs,
                                                      uint32_t* __restrict__ tickets,
                                                      int64_t* __restrict__ err, int32_t xg) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < kTicketGroups * kTicketStride; i += blockDim.x) tickets[i] = 0;
  // xg > 1: the blocks of one residue b % xg (the same XCD under the
  // round-robin dispatch, MI355X_MICROARCH.md; speed only) take the bands
  // k == b % xg (mod xg), so each XCD's L2 holds the rule infos of its own
  // one or two bands instead of every band the whole grid is working on
  const int32_t grp = int32_t(blockIdx.x % unsigned(xg));
  const int64_t nb_g = (int64_t(gridDim.x) - grp + xg - 1) / xg;
  const int64_t lb = blockIdx.x / unsigned(xg);
  const int64_t nbands = (int64_t(K) - grp + xg - 1) / xg;  // this group's bands
  const int64_t NKg = nbands * N;
  // Two segments per wave, one per half-wave (consecutive nodes of a band),
  // software-pipelined: the kernel is latency-bound (segment bounds -> pair
  // rules -> rule infos -> records), so each iteration issues the bounds two
  // segment pairs ahead, the first round of pair rules one ahead and its own
  // rule infos together, and waits once.
  constexpr int L = 32;  // lanes per segment
  constexpr int P = kSegPairsPerLane;
  const int lane = threadIdx.x & 63, hl = lane & (L - 1);
  // every half-wave walks its own run of `per` consecutive segments (in band
  // order): the blocks resident at any time cover a few consecutive bands, so
  // their rule infos stay in L2 even when the grid is many times the blocks
  // the CUs hold at once (a grid-stride walk spread the resident blocks over
  // ~20 bands: half the info gathers missed L2, 72 GB per config-4 window)
  const int64_t Hg = nb_g * (blockDim.x >> 6) * 2;
  const int64_t per = (NKg + Hg - 1) / Hg;
  const int64_t hid = (lb * int64_t(blockDim.x >> 6) + (threadIdx.x >> 6)) * 2 + (lane >> 5);
  const uint32_t below = (1u << hl) - 1u;  // lanes of this half before this one
  struct Seg {
    int64_t s, p0, p1;
  };
  auto bounds = [&](int64_t u) -> Seg {
    const int64_t t = hid * per + u;
    Seg g{-1, 0, 0};
    if (u < per && t < NKg) {
      const int32_t i = int32_t(t / N), n = int32_t(t - int64_t(i) * N);
      const int32_t k = grp + xg * i;
      g.s = int64_t(n) * K + k;
      g.p0 = seg_pair[g.s];
      g.p1 = seg_pair[g.s + 1];
    }
    return g;
  };
  // pair u*L + hl of round pc: every load and record store instruction covers
  // consecutive pairs / records
  auto rules = [&](const Seg& g, int32_t pc, int32_t (&r)[P]) {
#pragma unroll
    for (int u = 0; u < P; u++) {
      const int64_t pp = g.p0 + pc + u * L + hl;
      r[u] = pp < g.p1 ? nt_rule[pp] : -1;
    }
  };
  Seg cur = bounds(0), nxt = bounds(1);
  int32_t r[P], rn[P];
  rules(cur, 0, r);
  for (int64_t u = 0; u < per; u++) {
    const Seg nn = bounds(u + 2);  // two ahead
    rules(nxt, 0, rn);                   // the next pair's first round
    int64_t run = 0;  // events of the segment so far
    int32_t nrec = 0;
    const int32_t len = int32_t(cur.p1 - cur.p0);
    const int32_t rounds_len = max(__builtin_amdgcn_readlane(len, 0), __builtin_amdgcn_readlane(len, 32));
    for (int32_t pc = 0; pc < rounds_len; pc += L * P) {
      if (pc > 0) rules(cur, pc, r);  // segments of more than L*P pairs
      RuleInfo g[P];
#pragma unroll
      for (int u = 0; u < P; u++)
        g[u] = r[u] >= 0 ? info[r[u]] : RuleInfo{0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < P; u++) {
        // events before this pair: half-wave inclusive scan of the counts
        // (int32: a band holds < 2^30 events, k_rule_info checks)
        const int32_t incl = scan_halves(g[u].cnt);
        const int64_t d = run + (incl - g[u].cnt);
        const uint64_t ball = __ballot(g[u].cnt > 0);
        const uint32_t ne = uint32_t(lane < 32 ? ball : ball >> 32);  // this half's non-empty pairs
        if (g[u].cnt > 0) {
          const int64_t at = cur.p0 + nrec + __popc(ne & below);
          const int64_t x = int64_t(g[u].first) - d * g[u].st;
          const bool prog = g[u].st != 0 && x >= INT32_MIN && x <= INT32_MAX;
          recs[at] = PairRec{r[u], int32_t(d), int32_t(prog ? x : int64_t(g[u].off) - d), prog ? g[u].st : 0};
        }
        run += half_total(incl);
        nrec += __popc(ne);
      }
    }
    if (hl == 0 && cur.s >= 0) {
      seg_cnt[cur.s] = run;
      seg_nrec[cur.s] = nrec;
      if (run > (int64_t(1) << 30)) err[0] = 1;
    }
    cur = nxt;
    nxt = nn;
#pragma unroll
    for (int u = 0; u < P; u++) r[u] = rn[u];
  }
}

// node_off[n] = seg_pos[n*K] (n <= N); the total is also stored to res
__global__ void k_node_off_from_seg(const int64_t* __restrict__ seg_pos, int32_t N, int32_t K,
                                    int64_t* __restrict__ node_off, int64_t* __restrict__ res) {
  const int64_t n = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (n > N) return;
  node_off[n] = seg_pos[n * K];
  if (n == N) res[0] = seg_pos[n * K];
}

__device__ __forceinline__ int64_t rl64n(int64_t v, int i) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), i));
  const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(uint64_t(v) >> 32)), i));
  return int64_t((uint64_t(hi) << 32) | lo);
}

// Output stores are nontemporal (streaming): plain stores keep the written
// lines in the XCD's L2, and nt stores were the fastest on one box (pernode
// writer 2.36 ms vs 2.60 sc1 -- relaxed agent-scope atomic stores -- and 2.71
// plain, profiles/r02_ab_node_store.json).  V & 2 (diagnostic build): no store.
template <int V, class T>
__device__ __forceinline__ void out_store(T* p, T v) {
  if (V & 2) {
    asm volatile("" ::"v"(v));
    return;
  }
  __builtin_nontemporal_store(v, p);
}
// Writer task order: 0 band-major (every node's segment of band 0, then band
// 1, ...: a band's fire lists stay in L2 for the gathers), 1 node-major (the
// segments of one node in turn: the concurrent write fronts stay in a few
// nodes' lists).  Rule-ordered lists are written node-major (same-box A/B,
// profiles/r05_ab_writer_order.txt: config 3 150.4 -> 146.9 ms, pernode
// -3 %, config 4 per node -2 %) unless a node has many bands (node_major_for);
// the time-order writer's packed words band-major (node-major: config 3 in
// time order +1 %, pernode equal).
constexpr int kNodeMajorDefault = 1;
constexpr int kNodeMajorOrdered = 0;  // the time-order writer (packed words / 16-bit offsets)
// rule-ordered lists with many bands per node go band-major: a node-major
// sweep of K bands spreads the gathers over every band's fire lists, while
// band-major keeps one band's in L2 (same-box A/B, profiles/r06_ab_writer_order_bands.txt:
// config 4 per node, K = 305, 5 windows 201.8-203.4 -> 195.8-197.3 ms; config 3
// and pernode, K = 31, stay node-major: 140.4 vs 152.6 ms, 3.14-3.18 vs 3.20)
constexpr int32_t kNodeBandMajorK = 128;
inline int node_major_for(int32_t K) { return K >= kNodeBandMajorK ? 0 : kNodeMajorDefault; }
// 8 ticket groups, each spread across the 8 XCDs as k_write_cf's (same-box
// A/Bs, profiles/r06_ab_node_writer_groups.txt: config 3 174.9 -> 170.7 ms per
// step, node writer 152.1 -> 146.7, pernode equal;
// profiles/r06_ab_ticket_groups_pn.txt: pernode node writer 2.45 -> 2.29 ms
// with 8 instead of 32, config 3 -1.5 %)
constexpr int kNodeGroups = 8 < kTicketGroups ? 8 : kTicketGroups;

// One (node, band) segment's events from its records (k_seg_records), in
// output position order, 64-event blocks at a time: put(q, val, rv) for the
// lanes whose position q (relative to the 64-aligned abase) is in the
// segment -- the whole block, or the lanes inside the segment at its edges.
// The body of k_node_write (the bucket writer of commit 7beb946 shared it).
//   runs   a block one record owns entirely (no record starts inside it) is
//          stored straight from that record: a progression's fires are
//          t0 + x + p * stride, so a run of such blocks costs two stores and
//          an add per block (other records: one gather per block);
//   one()  a block where records start, and the chunk's first and last blocks
//          (shared with the neighbouring chunk, or at the segment's edges):
//          the records starting in it mark their first lane in an LDS row
//          (tagged, no clearing); lane l's record = (records starting before
//          the block: one ballot over the sorted starts) - 1 + popcount(marks
//          at lanes <= l); its x, stride and rule come from that record's lane
//          (ds_bpermute).  A block shared with the next chunk is carried in
//          registers; only blocks at segment edges are stored partially.
// Gathers are waited for where they are issued: a wave's loads and stores
// retire in issue order, so a wait after a join would drain its stores on
// every block.  V (diagnostic build only): 1 = no gather (the index as the
// value), 2 = no stores, 8 = no rule-index stores.
template <int V, class Put>
__device__ __forceinline__ void node_segment(int64_t p0, int32_t nrec, int32_t q_lo, int32_t q_hi,
                                             const int64_t* __restrict__ tb, const PairRec* __restrict__ recs,
                                             int64_t t0, uint32_t* marks, uint32_t& tag, uint64_t le, Put&& put) {
  const int lane = threadIdx.x & 63;
  int32_t pq = -1, prule = 0;  // a block carried into the next chunk
  int64_t ptime = 0;
  // records in chunks of 64 (lane i: record i), the next chunk in flight
  // (an unconditional load at a clamped index: a load under a branch is
  // waited for at the branch's end, so the prefetch would not stay in flight)
  PairRec nx;
  int32_t nx_end = q_hi;
  auto fetch = [&](int32_t w) {
    nx = recs[p0 + (w + lane < nrec ? w + lane : nrec - 1)];
    // the chunk ends where the next one's first record starts
    nx_end = w + 64 < nrec ? recs[p0 + w + 64].dst + q_lo : q_hi;
  };
  fetch(0);
  for (int32_t w = 0; w < nrec; w += 64) {
    // q of first event; x and stride of the record (k_seg_records)
    const int32_t rr = nx.rule, dst = nx.dst + q_lo, dlt = nx.x, sst = nx.st, we = nx_end;
    const int nc = nrec - w < 64 ? nrec - w : 64;
    const int32_t qw = __builtin_amdgcn_readlane(dst, 0);
    if (w + 64 < nrec) fetch(w + 64);
    const bool live = lane < nc;
    auto one = [&](int32_t b) {
      tag++;
      const bool mark = live && dst >= b && dst < b + 64;
      marks[mark ? dst - b : 64 + lane] = tag;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int32_t q = b + lane;
      const uint64_t M = __ballot(marks[lane] == tag);
      const int before = __popcll(__ballot(live && dst < b));
      int own = before - 1 + __popcll(M & le);
      own = own < 0 ? 0 : (own >= nc ? nc - 1 : own);
      const int32_t dl = __builtin_amdgcn_ds_bpermute(own << 2, dlt);
      const int32_t sv = __builtin_amdgcn_ds_bpermute(own << 2, sst);
      int32_t rv = __builtin_amdgcn_ds_bpermute(own << 2, rr);
      const bool in = q >= qw && q < we;
      int64_t val = in && sv != 0 ? t0 + int64_t(dl) + int64_t(q - q_lo) * sv : 0;
      const int32_t gi = in && sv == 0 ? q + dl - q_lo : -1;
      if (__ballot(gi >= 0)) {  // waited for here, not after the branch
        if (gi >= 0) val = (V & 1) ? int64_t(gi) : tb[gi];
        asm volatile("" : "+v"(val));
      }
      if (b == pq) {  // lanes of the previous chunk
        val = q < qw ? ptime : val;
        rv = q < qw ? prule : rv;
      }
      if (b + 64 <= we || we == q_hi) {  // complete, or the segment's last block
        if ((b >= q_lo && b + 64 <= q_hi) || (q >= q_lo && q < q_hi)) {  // whole, or a segment edge
          put(q, val, rv);
        }
        pq = -1;
      } else {  // carried into the next chunk
        pq = b;
        ptime = val;
        prule = rv;
      }
    };
    const int32_t b0 = qw & ~63, bl = we & ~63;
    if (qw & 63) one(b0);
    for (int32_t b = (qw + 63) & ~63; b < bl;) {
      const int o = __popcll(__ballot(live && dst <= b)) - 1;  // owner of lane 0 (dst[0] = qw <= b)
      const int32_t e = o + 1 < nc ? __builtin_amdgcn_readlane(dst, o + 1) : we;
      if (e < b + 64) {  // a record starts inside
        one(b);
        b += 64;
        continue;
      }
      const int32_t bend = (e & ~63) < bl ? (e & ~63) : bl;  // blocks [b, bend) all o's
      const int32_t dl = __builtin_amdgcn_readlane(dlt, o), sv = __builtin_amdgcn_readlane(sst, o);
      const int32_t rv = __builtin_amdgcn_readlane(rr, o);
      if (sv != 0) {
        int64_t val = t0 + int64_t(dl) + int64_t(b + lane - q_lo) * sv;
        const int64_t step = int64_t(64) * sv;
        for (; b < bend; b += 64, val += step) {
          put(b + lane, val, rv);
        }
      } else {
        for (; b < bend; b += 64) {
          const int32_t gi = b + lane + dl - q_lo;
          int64_t val = (V & 1) ? int64_t(gi) : tb[gi];
          asm volatile("" : "+v"(val));
          put(b + lane, val, rv);
        }
      }
    }
    if ((we & 63) && (bl != b0 || !(qw & 63))) one(bl);
  }
}

// Per-node lists, one (node, band) segment per wave task, tasks taken by
// ticket in the given order; a segment's blocks are filled by node_segment.
// OUT (windows <= 4096 s whose lists the time-order tile sort reads next):
// kInTimes int64 times + int32 rules; kIn16 the times as 16-bit offsets
// t - t0 - 1 (2 B per event instead of 8); kInPacked one word per event,
// offset << 20 | rule, into out_rule (4 B per event instead of 2 + 4; rule
// indices < 2^20)
template <int V, int OUT = kInTimes>
__global__ __launch_bounds__(256) void k_node_write(
    const int64_t* __restrict__ seg_pair, const int64_t* __restrict__ seg_pos,
    const int32_t* __restrict__ seg_nrec, const PairRec* __restrict__ recs, int64_t t0,
    const int64_t* __restrict__ rule_off, const int64_t* __restrict__ times, int32_t N, int32_t K,
    int32_t B, int64_t cap, uint32_t* __restrict__ tickets, int64_t* __restrict__ out_time,
    int32_t* __restrict__ out_rule, int node_major) {
  // per wave one 128-slot mark row (slots 64..127: the writes of lanes that
  // mark nothing); tags only grow, so no clearing
  __shared__ uint32_t marks_all[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* marks = marks_all[wave];
  marks[lane] = 0u;
  uint32_t tag = 0;
  const int64_t NK = int64_t(N) * K;
  if (seg_pos[NK] > cap) return;  // output too small: the host grows it and relaunches
  const uint64_t le = (2ull << lane) - 1ull;  // lanes <= this one
  const int ng = int(gridDim.x) < kNodeGroups ? int(gridDim.x) : kNodeGroups;
  // every group across the 8 XCDs (cf. k_write_cf), when the grid gives
  // every group a block that way (a small grid: one group per block)
  const int grp = int(gridDim.x >= 8u * unsigned(ng) ? (blockIdx.x >> 3) % unsigned(ng) : blockIdx.x % unsigned(ng));
  auto take = [&]() -> int64_t {
    unsigned int t = 0;
    if (lane == 0) t = atomicAdd(tickets + grp * kTicketStride, 1u);
    return grp + int64_t(ng) * int64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(t))));
  };
  // a task's descriptor, loaded one task ahead by lanes 0..4
  auto desc = [&](int64_t t) -> int64_t {
    if (t >= NK) return 0;
    const int32_t k = node_major ? int32_t(t % K) : int32_t(t / N);
    const int32_t n = node_major ? int32_t(t / K) : int32_t(t - int64_t(k) * N);
    const int64_t s = int64_t(n) * K + k;
    switch (lane) {
      case 0: return seg_pair[s];
      case 1: return seg_nrec[s];
      case 2: return seg_pos[s];
      case 3: return seg_pos[s + 1];
      case 4: return rule_off[int64_t(k) * B];
      default: return 0;
    }
  };
  int64_t t = take();
  int64_t dsc = desc(t);
  while (t < NK) {
    const int64_t t_next = take();
    const int64_t dsc_next = desc(t_next);
    const int64_t p0 = rl64n(dsc, 0), o0 = rl64n(dsc, 2), o1 = rl64n(dsc, 3), band_lo = rl64n(dsc, 4);
    const int32_t nrec = int32_t(rl64n(dsc, 1));
    t = t_next;
    dsc = dsc_next;
    if (o0 == o1) continue;
    // segment-local 32-bit positions: q = output index - abase (abase 64-aligned)
    const int64_t abase = o0 & ~int64_t(63);
    const int32_t q_lo = int32_t(o0 - abase), q_hi = q_lo + int32_t(o1 - o0);
    const int64_t* __restrict__ tb = times + band_lo;
    int64_t* __restrict__ ot = out_time + abase;
    uint16_t* __restrict__ o16 = reinterpret_cast<uint16_t*>(out_time) + abase;
    int32_t* __restrict__ orl = out_rule + abase;
    auto put = [&](int32_t q, int64_t val, int32_t rv) {
      if constexpr (OUT == kInPacked) {
        out_store<V>(orl + q, int32_t((uint32_t(val - t0 - 1) << 20) | (uint32_t(rv) & 0xFFFFFu)));  // rule >> 20: per tile
        return;
      }
      if constexpr (OUT == kIn16) out_store<V>(o16 + q, uint16_t(val - t0 - 1));
      else out_store<V>(ot + q, val);
      if (!(V & 8)) out_store<V>(orl + q, rv);
    };
    node_segment<V>(p0, nrec, q_lo, q_hi, tb, recs, t0, marks, tag, le, put);
  }
}

// The writer for an output mode (kInTimes / kIn16 / kInPacked); variant: the
// diagnostic build's V of the kInTimes writer (CG_NODE_VARIANT: 1 no gather,
// 2 no stores, 3 neither, 8 no rule stores)
auto node_write_kernel(int out_mode, int variant) {
  if (out_mode == kInPacked) return &k_node_write<0, kInPacked>;
  if (out_mode == kIn16) return &k_node_write<0, kIn16>;
#ifdef CG_DIAG
  switch (variant) {
    case 1: return &k_node_write<1, kInTimes>;
    case 2: return &k_node_write<2, kInTimes>;
    case 3: return &k_node_write<3, kInTimes>;
    case 8: return &k_node_write<8, kInTimes>;
  }
#endif
  return &k_node_write<0, kInTimes>;
}

// persistent k_node_write grid: as many 4-wave blocks per CU as its register
// and LDS use let run at once (no block of the grid waits for a slot)
#ifndef CG_NODE_BPC
#define CG_NODE_BPC 0  // 0: as many as the occupancy allows (up to 8)
#endif
int node_write_blocks_per_cu() {
  if (CG_NODE_BPC > 0) return CG_NODE_BPC + 2;  // the pipelined windows leave two slots free
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, node_write_kernel(kInTimes, 0), 256, 0) != hipSuccess || n < 1)
    n = 4;
  return std::min(n, 8);
}

// Rules per band: the band's rule-major fire lists (E_band * 8 B) should sit
// in one XCD's 4 MiB L2 beside the write stream; a power of two, so the
// cached segment bounds stay valid across windows of similar volume.
#ifndef CG_BAND_MIN_RULES
#define CG_BAND_MIN_RULES 32768  // rules per band at least (profiles/r06_ab_band_floor.txt: config 3 146-151 -> 144 ms)
#endif
#ifndef CG_BAND_BYTES
#define CG_BAND_BYTES (1536 * 1024)
#endif
// largest fire-list span of a band of B rules (rule-major offsets): *out = max_k
// off[min((k+1)B, R)] - off[kB] (atomicMax; *out zeroed by the caller)
__global__ void k_band_max(const int64_t* __restrict__ off, int64_t R, int32_t B, unsigned long long* out) {
  const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  const int64_t a = k * B;
  if (a >= R) return;
  const int64_t b = a + B < R ? a + B : R;
  atomicMax(out, (unsigned long long)(off[b] - off[a]));
}

// band groups of k_seg_records: one per XCD when there are enough bands to
// balance them (else 1: every XCD's blocks walk the bands in order)
constexpr int32_t kSegXcdGroups = 8;
int32_t seg_xcd_groups(int32_t K) { return K >= 4 * kSegXcdGroups ? kSegXcdGroups : 1; }

// (at most 2^20 rules: the time-order pass cuts its tiles at multiples of
// 2^20 in rule index, found at band boundaries)
int32_t band_rules(int64_t R, int64_t E) {
  const double per_rule = double(std::max<int64_t>(E, 1)) * 8.0 / double(std::max<int64_t>(R, 1));
  int64_t B = int64_t(double(CG_BAND_BYTES) / per_rule);
  int64_t p = CG_BAND_MIN_RULES;
  while (p < B && p < R && p < (int64_t(1) << 20)) p <<= 1;
  return int32_t(std::max<int64_t>(p, 1024));
}

// ---- the per-window chain, shared by the synchronous and the pipelined
// entry points (which differ in the window's buffers, the stream, the
// writer's blocks per CU and its task order) ----

// Enqueues on st a window's rule infos, segment records, segment scan and
// node offsets (w.node_off, total to w.res_dev[0]) from its rule-major fire
// lists: offsets [R+1] and times (room for cap events) over the cached join
// (c->seg_pair, c->nt_rule; nnz pairs, K bands of B rules, N nodes).  The
// caller has set w.node_off and w.scan_tmp.  empty: nothing was counted (a
// pipelined window of no rules), every list is empty: memsets, no kernels.
int pn_records_enqueue(cg_ctx* c, PnWindow& w, const int64_t* offsets, const int64_t* times, int64_t cap, int64_t t0,
                       int64_t R, int32_t N, int32_t K, int32_t B, int64_t nnz, hipStream_t st, bool empty = false) {
  const int64_t NK = int64_t(N) * K;
  int rc;
  if ((rc = w.ensure_res()) || (rc = w.rule_info.ensure(rule_info_slots(R))) ||
      (rc = w.seg_cnt.ensure(std::max<int64_t>(NK, 1))) || (rc = w.seg_pos.ensure(NK + 1)) ||
      (rc = w.seg_nrec.ensure(std::max<int64_t>(NK, 1))) || (rc = w.recs.ensure(std::max<int64_t>(nnz, 1))) ||
      (rc = w.tickets.ensure(kTicketGroups * kTicketStride)))
    return rc;
  w.offsets = offsets, w.times = times, w.t0 = t0;
  w.N = N, w.K = K, w.B = B;
  w.res_host[0] = w.res_host[1] = w.res_host[2] = 0;  // (nothing of this window is in flight here)
  if (empty) {
    HIPCHK(hipMemsetAsync(w.seg_pos.p, 0, (NK + 1) * 8, st));
    HIPCHK(hipMemsetAsync(w.rule_info.p, 0, rule_info_slots(R) * sizeof(RuleInfo), st));
    if (NK > 0) HIPCHK(hipMemsetAsync(w.seg_cnt.p, 0, NK * 8, st));
  } else {
    if (R > 0)
      hipLaunchKernelGGL(k_rule_info, dim3(unsigned((R + kApRules - 1) / kApRules)), dim3(256), 0, st, offsets, times,
                         R, t0, B, cap, w.rule_info.p, w.res_dev + 1);
    if (NK > 0)
      hipLaunchKernelGGL(k_seg_records, dim3(gridn(NK, 4, 256 * 64)), dim3(256), 0, st, c->seg_pair.p, c->nt_rule.p,
                         offsets, w.rule_info.p, N, K, B, R, w.seg_cnt.p, w.seg_nrec.p, w.recs.p, w.tickets.p,
                         w.res_dev + 1, seg_xcd_groups(K));
  }
  if (NK > 0 || !empty) launch_scan64(w.seg_cnt.p, w.seg_pos.p, NK, w.scan_tmp, st);
  hipLaunchKernelGGL(k_node_off_from_seg, dim3(gridn(int64_t(N) + 1, 256, 1 << 30)), dim3(256), 0, st, w.seg_pos.p,
                     N, K, w.node_off, w.res_dev);
  return CG_OK;
}

// CG_NODE_VARIANT of the diagnostic build (node_write_kernel); 0 otherwise
int node_write_variant() {
#ifdef CG_DIAG
  static const int variant = [] {
    const char* e = getenv("CG_NODE_VARIANT");
    return e ? atoi(e) : 0;
  }();
  return variant;
#else
  return 0;
#endif
}

// Enqueues on st the writer of the window pn_records_enqueue prepared: its
// lists into c->node_time / c->node_rule (room for cap events; the kernel
// does nothing if the window holds more) in out_mode, tasks in node_major
// order, on a persistent grid of per_cu blocks per CU.
void pn_writer_enqueue(cg_ctx* c, const PnWindow& w, int out_mode, int node_major, int per_cu, int64_t cap,
                       hipStream_t st) {
#ifdef CG_DIAG
  // diagnostic overrides: blocks of 4 waves per CU, and the rule-ordered
  // writer's task order (see node_major_for)
  static const char* const env_per_cu = getenv("CG_NODE_BLOCKS_PER_CU");
  static const char* const env_order = getenv("CG_NODE_ORDER");
  if (env_per_cu) per_cu = std::max(1, atoi(env_per_cu));
  if (env_order && out_mode == kInTimes) node_major = atoi(env_order);
#endif
  const int64_t NK = int64_t(w.N) * w.K;
  const int nw_blocks = c->write_blocks / kWriteBlocksPerCU * per_cu;
  hipLaunchKernelGGL(node_write_kernel(out_mode, node_write_variant()),
                     dim3(unsigned(std::min<int64_t>(NK / 4 + 1, nw_blocks))), dim3(256), 0, st, c->seg_pair.p,
                     w.seg_pos.p, w.seg_nrec.p, w.recs.p, w.t0, w.offsets, w.times, w.N, w.K, w.B, cap, w.tickets.p,
                     c->node_time.p, c->node_rule.p, node_major);
}

// res[1] of a window set: a segment or a band outgrew the writer's 32-bit positions
std::string pn_size_error_msg(int32_t B) {
  return "per-node output: a (node, rule band) segment, or a band of " + std::to_string(B) +
         " consecutive rules, fires more than 2^30 times in this window (the writer's 32-bit band indices; "
         "narrow the time window)";
}

int per_node_locked(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                    const RulesStore& in, int mode, int64_t* n_events, int64_t* nnz_out) {
  if (int64_t(s->n) != in.n_rules)
    return cg_fail(CG_EINVAL, "specs count != rules n_rules");
  int64_t E = 0;
  int rc = expand_device_locked(c, s, z, t0, t1, &E);
  if (rc) return rc;
  int64_t nnz = 0;
  const int32_t N = in.n_nodes;
  const int64_t R = in.n_rules;
  hipStream_t st = c->st;
  const bool cached = in.serial != 0 && in.serial == c->pn_cache_serial && mode == c->pn_cache_mode;
  c->pn_E = 0;  // no readable result until this call succeeds
  c->pn_valid = false;
  c->pn_time_ordered = false;
  c->pn_R = R;
  (void)hipEventRecord(c->pev[0], st);
  if (cached) {
    nnz = c->pn_nnz;
  } else {
    c->pn_cache_serial = 0;  // the transpose buffers are about to change
    c->pn_K = 0;
    if ((rc = rule_nodes_locked(c, in, mode, &nnz))) return rc;
  }
  (void)hipEventRecord(c->pev[1], st);
  if (!cached && (rc = transpose_locked(c, nnz, N))) return rc;
  // segments (node, rule band): bounds cached per band width.  The writer's
  // band-relative indices are 32-bit: when the window holds more than 2^30
  // fires, bands whose fire lists pass 2^30 are halved (down to kApRules
  // rules; e.g. 1024 every-second rules over 13 days)
  int32_t B = band_rules(R, E);
  if (E > (int64_t(1) << 30) && R > 0) {
    if ((rc = c->cksum.ensure(1))) return rc;
    for (;;) {
      HIPCHK(hipMemsetAsync(c->cksum.p, 0, 8, st));
      hipLaunchKernelGGL(k_band_max, dim3(gridn((R + B - 1) / B, 256, 1 << 30)), dim3(256), 0, st,
                         c->rs.offsets.p, R, B, c->cksum.p);
      unsigned long long mx = 0;
      HIPCHK(hipMemcpyAsync(&mx, c->cksum.p, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (mx <= (1ull << 30) || B <= kApRules) break;
      B /= 2;
    }
  }
  const int32_t K = int32_t(std::max<int64_t>(1, (R + B - 1) / B));
  const int64_t NK = int64_t(N) * K;
  if ((rc = c->seg_pair.ensure(NK + 1)) || (rc = c->node_off.ensure(N + 1))) return rc;
  if ((rc = c->scan_tmp.ensure(std::max(c->scan_tmp.cap, scan_temp_bytes(NK))))) return rc;
  if (!(cached && c->pn_B == B && c->pn_K == K)) {
    hipLaunchKernelGGL(k_seg_bounds, dim3(gridn(NK + 1, 256, 1 << 30)), dim3(256), 0, st, c->nt_off.p,
                       c->nt_rule.p, N, K, B, c->seg_pair.p);
    c->pn_B = B;
    c->pn_K = K;
  }
  PnWindow& w = c->pn;
  w.node_off = c->node_off.p;
  w.scan_tmp = c->scan_tmp.p;
  if ((rc = pn_records_enqueue(c, w, c->rs.offsets.p, c->times.p, int64_t(c->times.cap), t0, R, N, K, B, nnz, st)))
    return rc;
  (void)hipEventRecord(c->pev[2], st);
  // the writer reads the total on the device and does nothing if it exceeds
  // the output capacity (first call or a larger result: grow, relaunch)
  static const int per_cu = node_write_blocks_per_cu();
  // (time, rule) order of a window <= 4096 s (the predicate of
  // order_by_time_locked's tile sort: bits <= 12, not LSD): the writer emits
  // 16-bit offsets t - t0 - 1 (or packed words) for the tile sort
  const bool off16 =
      c->node_order == CG_NODE_ORDER_TIME && t1 - t0 <= 4096 && node_write_variant() == 0 && !order_lsd_only();
  // packed words (offset << 20 | rule) when every rule index fits 20 bits
  const int in_mode = !off16 ? kInTimes : (pn_pack_ok(R) ? kInPacked : kIn16);
  const int node_major = off16 ? kNodeMajorOrdered : node_major_for(K);
  int64_t En = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    const int64_t cap = int64_t(std::min(c->node_time.cap, c->node_rule.cap));
    if (NK > 0 && cap > 0) pn_writer_enqueue(c, w, in_mode, node_major, per_cu, cap, st);
    (void)hipEventRecord(c->pev[3], st);
    if ((rc = cg_hip_check(hipGetLastError(), "per-node kernels"))) return rc;
    if ((rc = cg_hip_check(hipStreamSynchronize(st), "sync"))) return rc;
    En = w.res_host[0];
    if (w.res_host[1] != 0) return cg_fail(CG_ERANGE, pn_size_error_msg(B));
    if (En <= cap) break;
    // grow the output, reset the tickets the first launch consumed, rerun
    if ((rc = c->node_time.ensure(En)) || (rc = c->node_rule.ensure(En))) return rc;
    HIPCHK(hipMemsetAsync(w.tickets.p, 0, kTicketGroups * kTicketStride * 4, st));
    (void)hipEventRecord(c->pev[2], st);
  }
  (void)hipEventElapsedTime(&c->kt[KT_PN_JOIN], c->pev[0], c->pev[1]);
  (void)hipEventElapsedTime(&c->kt[KT_PN_TRANSPOSE], c->pev[1], c->pev[2]);
  (void)hipEventElapsedTime(&c->kt[KT_PN_WRITE], c->pev[2], c->pev[3]);
  c->pn_E = En;
  c->pn_valid = true;
  c->pn_nnz = nnz;
  c->pn_N = N;
  c->pn_t0 = t0;
  c->pn_t1 = t1;
  c->pn_cache_serial = in.serial;
  c->pn_cache_mode = mode;
  *n_events = En;
  *nnz_out = nnz;
  // (time, rule) order: the tile sort + merge (or, past 4096 s, the LSD
  // passes) after the writer; if it fails nothing is readable (the lists may
  // hold the writer's 16-bit offsets)
  if (c->node_order == CG_NODE_ORDER_TIME) {
    if ((rc = order_by_time_locked(c, in_mode))) {
      c->pn_E = 0;
      c->pn_valid = false;
      *n_events = 0;
    }
    return rc;
  }
  c->kt[KT_TIME_ORDER] = 0.f;
  return CG_OK;
}

}  // namespace

// ---- pipelined per-node windows -------------------------------------------
// A node scheduler's tick loop (node/node.go:121-158 filtering every job,
// node/cron/cron.go:210-275 firing them) asks for consecutive windows of every
// node's list.  The synchronous entry point runs a window's expansion, records
// and writer in series with two host syncs; here window k+1's rule-major
// expansion, rule infos, segment records and node offsets run on the second
// stream (into set (k+1) % 3) while window k's k_node_write streams on the
// first.  The rule->node join, its transpose, the band width and the segment
// bounds come from an earlier synchronous call on the same rule set and mode.

namespace {

void pn_check_set(cg_ctx* c, PnAsyncSet& a) {
  if (!a.pending) return;
  a.pending = false;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a.nw0, a.nw1) == hipSuccess) {
    c->nw_ms_sum += ms;
    c->nw_n++;
  }
  const int64_t E = a.rm.res_host[0], En = a.w.res_host[0];
  c->pa_en_sum += En;
  if (c->pa_rc) return;  // keep the first error
  const unsigned long long stuck = static_cast<unsigned long long>(a.rm.res_host[1]);
  if (stuck != ~0ULL) {
    c->pa_rc = CG_ERANGE;
    c->pa_msg = stuck_msg(stuck);
  } else if (E > a.rm_cap) {
    c->pa_rc = CG_ECAPACITY;
    c->pa_msg = "per-node async window (" + std::to_string(a.t0) + ", " + std::to_string(a.t1) + "]: " +
                std::to_string(E) + " rule-major events exceed the capacity " + std::to_string(a.rm_cap) +
                " (run a synchronous per-node call on a window this large first)";
  } else if (a.w.res_host[2] != 0) {
    c->pa_rc = CG_EHIP;
    c->pa_msg = kOrderCheckMsg;
  } else if (a.w.res_host[1] != 0) {
    c->pa_rc = CG_ERANGE;
    c->pa_msg = pn_size_error_msg(a.w.B);
  } else if (En > a.node_cap) {
    c->pa_rc = CG_ECAPACITY;
    c->pa_msg = "per-node async window (" + std::to_string(a.t0) + ", " + std::to_string(a.t1) + "]: " +
                std::to_string(En) + " node events exceed the output capacity " + std::to_string(a.node_cap) +
                " (run a synchronous per-node call on a window this large first)";
  }
}

int pn_ensure_async(cg_ctx* c) {
  int rc = ensure_async(c);  // the second stream
  if (rc) return rc;
  for (PnAsyncSet& a : c->pns) {
    if (a.written) continue;
    HIPCHK(hipEventCreateWithFlags(&a.side_done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&a.written, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&a.nw0, hipEventDisableSystemFence));
    HIPCHK(hipEventCreateWithFlags(&a.nw1, hipEventDisableSystemFence));
  }
  return CG_OK;
}

}  // namespace

bool pn_async_pending(const cg_ctx* c) {
  for (const PnAsyncSet& a : c->pns)
    if (a.pending) return true;
  return false;
}

int pn_async_drain(cg_ctx* c) {
  if (!pn_async_pending(c)) return CG_OK;
  HIPCHK(hipStreamSynchronize(c->st));
  for (PnAsyncSet& a : c->pns) pn_check_set(c, a);
  return CG_OK;
}

extern "C" {

int cg_expand_per_node_rules_device_async(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                                          const cg_rules* rules, int mode) {
  if (!c || !s || !z || !rules) return cg_fail(CG_EINVAL, "cg_expand_per_node_rules_device_async: null");
  if (rules->ctx != c) return cg_fail(CG_EINVAL, "rule set uploaded on another context");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  const RulesStore& in = rules->st;
  if (int64_t(s->n) != in.n_rules) return cg_fail(CG_EINVAL, "specs count != rules n_rules");
  if (!(in.serial != 0 && in.serial == c->pn_cache_serial && mode == c->pn_cache_mode && c->pn_K > 0))
    return cg_fail(CG_EINVAL, "cg_expand_per_node_rules_device_async: run cg_expand_per_node_rules_device once "
                              "on this rule set and exclude mode first (rule->node join, bands, capacity)");
  if (t1 - t0 > CG_MAX_HORIZON || t0 < -(int64_t(1) << 45) || t1 > (int64_t(1) << 45))
    return cg_fail(CG_ERANGE, "horizon must satisfy t1 - t0 <= CG_MAX_HORIZON (40 years)");
  if (async_pending(c))  // their only readable result would be lost below
    return cg_fail(CG_EINVAL, "pipelined rule-major calls pending (call cg_expand_wait first)");
  const int64_t rm_cap = int64_t(c->times.cap);
  const int64_t node_cap = int64_t(std::min(c->node_time.cap, c->node_rule.cap));
  if (rm_cap == 0 || node_cap == 0) return cg_fail(CG_ECAPACITY, "no output capacity yet (run a synchronous call)");
  int rc = pn_ensure_async(c);
  if (rc) return rc;
  // the rule-major result and the time-order records no longer describe a result
  c->as_last = -1;
  c->times_last = 0;
  c->last_R = 0;
  c->last_E = 0;
  c->res_gen++;
  const int k = c->pa_next;
  PnAsyncSet& a = c->pns[k];
  // the set was last used kPnSets calls ago: its writer must be done
  HIPCHK(hipEventSynchronize(a.written));
  pn_check_set(c, a);
  const int32_t N = in.n_nodes, K = c->pn_K, B = c->pn_B;
  const int64_t R = in.n_rules, NK = int64_t(N) * K, nnz = c->pn_nnz;
  hipStream_t sc = c->st_cs, st = c->st;
  const bool timed = c->node_order == CG_NODE_ORDER_TIME;
  c->pn_R = R;
  if (timed && t1 - t0 > 4096)
    return cg_fail(CG_EINVAL, "pipelined per-node windows in time order: windows of at most 4096 s");
  bool empty = false;
  if ((rc = run_set_count_scan(a.rm, s, z, t0, t1, rm_cap, sc, nullptr, &empty))) return rc;
  if ((rc = a.times.ensure(std::max<int64_t>(rm_cap, 1))) || (rc = a.node_off.ensure(int64_t(N) + 1)) ||
      (rc = a.seg_tmp.ensure(scan_temp_bytes(std::max<int64_t>(NK, 1)))))
    return rc;
  // (empty: no rules, every list empty.)  The whole persistent grid: beside
  // the previous window's per-node writer only its free block slots run, and a
  // smaller grid left this latency-bound writer with fewer waves (same-box
  // A/B, profiles/r03_ab_pn_side.json: a quarter grid 3.21, a half 3.13, the
  // whole 3.12 ms per pernode step)
  if (!empty) run_set_write_enqueue(a.rm, s, rm_cap, a.times.p, c->write_blocks, sc);
  PnWindow& w = a.w;
  w.node_off = a.node_off.p;
  w.scan_tmp = a.seg_tmp.p;
  if ((rc = pn_records_enqueue(c, w, a.rm.offsets.p, a.times.p, rm_cap, t0, R, N, K, B, nnz, sc, empty))) return rc;
  HIPCHK(hipEventRecord(a.side_done, sc));
  // the writer after the previous window's writer, once this window's records are built
  HIPCHK(hipStreamWaitEvent(st, a.side_done, 0));
  (void)hipEventRecord(a.nw0, st);
  if (NK > 0 && !empty) {
    // two block slots per CU fewer than the synchronous path's persistent
    // grid: the next window's count, records and offsets (second stream) get
    // wave slots beside this writer instead of waiting for it to retire
    static const int per_cu = std::max(1, node_write_blocks_per_cu() - 2);
    if (timed) {  // packed words (or 16-bit offsets), then the tile sort + merge on the same stream
      const int in_mode = pn_pack_ok(R) ? kInPacked : kIn16;
      pn_writer_enqueue(c, w, in_mode, kNodeMajorOrdered, per_cu, node_cap, st);
      if ((rc = order_merge_enqueue(c, a.node_off.p, N, node_cap, t0, t1 - t0, st, in_mode, w.res_dev + 2,
                                    TileCut{w.seg_pos.p, K, B, R})))
        return rc;
    } else {
      pn_writer_enqueue(c, w, kInTimes, node_major_for(K), per_cu, node_cap, st);
    }
  }
  (void)hipEventRecord(a.nw1, st);
  HIPCHK(hipEventRecord(a.written, st));
  HIPCHK(hipGetLastError());
  a.pending = true;
  a.timed = timed;
  a.t0 = t0;
  a.t1 = t1;
  a.rm_cap = rm_cap;
  a.node_cap = node_cap;
  a.N = N;
  c->pa_next = (k + 1) % cg_ctx::kPnSets;
  c->pa_last = k;
  c->pn_E = 0;  // nothing readable until cg_expand_per_node_wait
  c->pn_valid = false;
  return CG_OK;
}

int cg_expand_per_node_wait(cg_ctx* c, int64_t* n_events, int64_t* n_events_all) {
  if (!c) return cg_fail(CG_EINVAL, "cg_expand_per_node_wait: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int rc = pn_async_drain(c);
  if (rc) return rc;
  if (c->nw_n > 0) c->kt[KT_PN_WRITE] = float(c->nw_ms_sum / c->nw_n);  // mean per-node writer time of the calls checked
  c->nw_ms_sum = 0;
  c->nw_n = 0;
  const int rc_async = c->pa_rc;
  const std::string msg = c->pa_msg;
  c->pa_rc = 0;
  c->pa_msg.clear();
  int64_t En = 0;
  if (c->pa_last >= 0) {
    PnAsyncSet& a = c->pns[c->pa_last];
    En = a.w.res_host[0];
    if (!rc_async) {  // the last window becomes the readable per-node result
      if ((rc = c->node_off.ensure(int64_t(a.N) + 1))) return rc;
      HIPCHK(hipMemcpyAsync(c->node_off.p, a.node_off.p, (int64_t(a.N) + 1) * 8, hipMemcpyDeviceToDevice, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
      c->pn_E = En;
      c->pn_valid = true;
      c->pn_time_ordered = a.timed;
      c->pn_N = a.N;
      c->pn_t0 = a.t0;
      c->pn_t1 = a.t1;
    }
    c->pa_last = -1;
  }
  if (n_events) *n_events = rc_async ? 0 : En;
  if (n_events_all) *n_events_all = c->pa_en_sum;
  c->pa_en_sum = 0;
  if (rc_async) return cg_fail(rc_async, msg);
  return CG_OK;
}

int cg_expand_per_node_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                              const cg_rules_in* rules, int mode, int64_t* n_events, int64_t* nnz) {
  if (!c || !s || !z || !rules || !n_events || !nnz)
    return cg_fail(CG_EINVAL, "cg_expand_per_node_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  if ((rc = upload_rules(rules, &c->rules, c->st))) return rc;
  return per_node_locked(c, s, z, t0, t1, c->rules, mode, n_events, nnz);
}

int cg_expand_per_node_rules_device(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0,
                                    int64_t t1, const cg_rules* rules, int mode, int64_t* n_events,
                                    int64_t* nnz) {
  if (!c || !s || !z || !rules || !n_events || !nnz)
    return cg_fail(CG_EINVAL, "cg_expand_per_node_rules_device: null");
  if (rules->ctx != c) return cg_fail(CG_EINVAL, "rule set uploaded on another context");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  return per_node_locked(c, s, z, t0, t1, rules->st, mode, n_events, nnz);
}

int cg_expand_per_node(cg_ctx* c, const cg_specs* s, const cg_zone* z, int64_t t0, int64_t t1,
                       const cg_rules_in* rules, int mode, cg_node_csr* out) {
  if (!c || !s || !z || !rules || !out) return cg_fail(CG_EINVAL, "cg_expand_per_node: null");
  std::lock_guard<std::mutex> g(c->mu);
  (void)hipGetLastError();  // clear a stale error so launch checks see only their own
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  int64_t En = 0, nnz = 0;
  if ((rc = upload_rules(rules, &c->rules, c->st))) return rc;
  if ((rc = per_node_locked(c, s, z, t0, t1, c->rules, mode, &En, &nnz))) return rc;
  out->n_events = En;
  out->nnz = nnz;
  if (out->node_off &&
      (rc = cg_hip_check(hipMemcpy(out->node_off, c->node_off.p, size_t(rules->n_nodes + 1) * 8,
                                   hipMemcpyDeviceToHost), "copy node_off")))
    return rc;
  if (out->time || out->rule) {
    if (out->cap < En) return cg_fail(CG_ECAPACITY, "per-node buffers too small; see n_events");
    if (En && out->time &&
        (rc = cg_hip_check(hipMemcpy(out->time, c->node_time.p, size_t(En) * 8, hipMemcpyDeviceToHost),
                           "copy time")))
      return rc;
    if (En && out->rule &&
        (rc = cg_hip_check(hipMemcpy(out->rule, c->node_rule.p, size_t(En) * 4, hipMemcpyDeviceToHost),
                           "copy rule")))
      return rc;
  }
  return CG_OK;
}

int cg_node_result_device(cg_ctx* c, const int64_t** d_node_off, const int64_t** d_time,
                          const int32_t** d_rule, int64_t* n_events) {
  if (!c) return cg_fail(CG_EINVAL, "cg_node_result_device: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  if (d_node_off) *d_node_off = c->node_off.p;
  if (d_time) *d_time = c->node_time.p;
  if (d_rule) *d_rule = c->node_rule.p;
  if (n_events) *n_events = c->pn_E;
  return CG_OK;
}

int cg_node_result_bands(cg_ctx* c, int32_t* rules_per_band, int32_t* n_bands) {
  if (!c) return cg_fail(CG_EINVAL, "cg_node_result_bands: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (c->pn_K == 0) return cg_fail(CG_EINVAL, "cg_node_result_bands: no synchronous per-node call yet");
  if (rules_per_band) *rules_per_band = c->pn_B;
  if (n_bands) *n_bands = c->pn_K;
  return CG_OK;
}

int cg_node_result_copy(cg_ctx* c, int64_t* node_off, int64_t* time, int32_t* rule, int64_t cap) {
  if (!c) return cg_fail(CG_EINVAL, "cg_node_result_copy: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  (void)hipGetLastError();
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  if (node_off && (rc = cg_hip_check(hipMemcpy(node_off, c->node_off.p, size_t(c->pn_N + 1) * 8,
                                               hipMemcpyDeviceToHost), "copy node_off")))
    return rc;
  if (time || rule) {
    if (cap < c->pn_E) return cg_fail(CG_ECAPACITY, "per-node buffers too small; see n_events");
    if (c->pn_E && time &&
        (rc = cg_hip_check(hipMemcpy(time, c->node_time.p, size_t(c->pn_E) * 8, hipMemcpyDeviceToHost),
                           "copy time")))
      return rc;
    if (c->pn_E && rule &&
        (rc = cg_hip_check(hipMemcpy(rule, c->node_rule.p, size_t(c->pn_E) * 4, hipMemcpyDeviceToHost),
                           "copy rule")))
      return rc;
  }
  return CG_OK;
}

int cg_node_result_copy_range(cg_ctx* c, int64_t first, int64_t count, int64_t* time, int32_t* rule) {
  if (!c || (count && !time && !rule)) return cg_fail(CG_EINVAL, "cg_node_result_copy_range: null");
  std::lock_guard<std::mutex> g(c->mu);
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  (void)hipGetLastError();
  int rc = cg_hip_check(hipSetDevice(c->device), "hipSetDevice");
  if (rc) return rc;
  if (first < 0 || count < 0 || first + count > c->pn_E)
    return cg_fail(CG_EINVAL, "range outside the last per-node result");
  if (count && time &&
      (rc = cg_hip_check(hipMemcpy(time, c->node_time.p + first, size_t(count) * 8, hipMemcpyDeviceToHost),
                         "copy time")))
    return rc;
  if (count && rule &&
      (rc = cg_hip_check(hipMemcpy(rule, c->node_rule.p + first, size_t(count) * 4, hipMemcpyDeviceToHost),
                         "copy rule")))
    return rc;
  return CG_OK;
}

}  // extern "C"
