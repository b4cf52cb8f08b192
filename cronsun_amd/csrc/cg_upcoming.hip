// cg_upcoming.hip -- the next k entries of a dispatcher table in byTime order
// on gfx950: Cron.Entries() (node/cron/cron.go:166-174) cut to its first k
// firing entries, cluster-wide or for one node's row of the bound join.
//
// The reference sorts the whole entry list on every wake (sort.Sort(byTime),
// cron.go:62-79,220) and Entries() hands that list out.  Here nothing is
// sorted but the answer: a radix select over the order key of Next finds the
// cut, an ordered compaction collects the entries at or before it, and only
// those (at most kUpCap pairs) are sorted.
//
// Candidates: entry i of the table, or entry j of a node's row
// nt_rule[nt_off[n] ..) with Next gathered; firing when next_key(Next) != ~0
// and Next <= until.  Every key is taken relative to `base`, the key of the
// dispatcher's effective time (the minimum over all firing entries, which the
// host holds): off = key - base >= 0.
//
//   select    k_up_hist, log mode: one pass bins every candidate by the highest
//             set bit of off (65 bins), so a table whose Next values sit
//             within days of the effective time lands its cut in a bin a few
//             bits wide whatever the absolute times are.  The host picks the
//             bin [lo, lo + 2^w) holding the k-th entry; while more entries
//             than the sort takes lie at or before that bin's end, a digit
//             pass (k_up_hist, 8 bits of off - lo) narrows it.  A bin one
//             value wide is the k-th key itself and its ties.  Blocks keep a
//             histogram in LDS over the tiles they stride and write one row
//             each; k_up_colsum adds the rows per bin.  No global atomics.
//             Worst case: 1 + ceil(63 / 8) = 9 histogram passes.
//   compact   k_up_count / scan / k_up_write: the entries below lo, and of
//             those inside the bin the first r in candidate order (all of
//             them, or the ties the cut takes), in ascending candidate order
//             = ascending slot.  Tiles that hold none are skipped unread.
//   sort      at most kUpSmall entries: one block ranks them in LDS.  More:
//             the transpose's stable LSD passes (k_rs_hist / k_rs_scatter) on
//             31-bit chunks of off, least significant first, over a
//             permutation.  Both are stable, so equal Next values stay in
//             ascending slot order; the first n_out are gathered with Prev.
// So a call streams the candidates 1 + d times for the select (d <= 8 digit
// passes), once for the count and at most once more for the write: 11 passes
// at worst, 3 where the first bin already is narrow enough.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "cg_api_internal.h"
#include "cg_dispatcher.h"

using namespace cg;

namespace {

constexpr int kUpTile = kDispatchTile;  // candidates per tile (count / write: one block each)
constexpr int kUpIter = kUpTile / 256;
constexpr int kUpWords = kUpTile / 64;  // wave words per tile, in candidate order
constexpr int kUpBins = 256;
constexpr int kUpLogBins = 65;
// grid cap of a histogram pass: a tile per block up to 16.7M candidates, as
// k_dispatch_scan runs (a block that strides tiles waits for each tile's loads)
constexpr int kUpHistBlocks = 4096;
constexpr int64_t kUpCap = 2 * int64_t(CG_UPCOMING_MAX);  // entries the compaction may collect
constexpr int64_t kUpSmall = 1024;   // sorted by one block in LDS
constexpr uint64_t kSign = uint64_t(1) << 63;

// What the passes select by.  A candidate with off = key - base <= uoff is
// BELOW when off < lo and IN when (off - lo) >> w == 0 (w == 64: every
// off >= lo).  Histogram bin of an IN candidate: log mode, the bit length of
// off - lo; else (off - lo) >> shift.
struct UpSel {
  unsigned long long base, uoff, lo, r;  // r: IN candidates taken, in candidate order
  int32_t w, shift, log;
};

// next_key of cg_kernels.hip: the order of Next under byTime, ~0 = not firing
__device__ __forceinline__ unsigned long long up_key(int64_t t) {
  return (t == CG_ZERO_TIME || t == CG_NO_PROGRESS) ? ~0ull : (uint64_t(t) ^ kSign);
}

enum { kNone = 0, kBelow = 1, kIn = 2 };

// -> class of a candidate; *d = off - lo of an IN one
__device__ __forceinline__ int up_class(int64_t t, const UpSel& s, unsigned long long* d) {
  const unsigned long long key = up_key(t);
  if (key == ~0ull || key < s.base) return kNone;
  const unsigned long long off = key - s.base;
  if (off > s.uoff) return kNone;
  if (off < s.lo) return kBelow;
  *d = off - s.lo;
  return (s.w >= 64 || (*d >> s.w) == 0) ? kIn : kNone;
}

// Next of candidate i (row: a node's slots; else slot i), the zero time past
// the end or for a slot outside the table
__device__ __forceinline__ int64_t up_load(const int64_t* __restrict__ next, const int32_t* __restrict__ row,
                                           int64_t M, int64_t n_slots, int64_t i) {
  if (i >= M) return CG_ZERO_TIME;
  if (!row) return __builtin_nontemporal_load(next + i);
  const int64_t s = row[i];
  return s >= 0 && s < n_slots ? next[s] : CG_ZERO_TIME;
}

__global__ __launch_bounds__(256) void k_up_hist(const int64_t* __restrict__ next,
                                                  const int32_t* __restrict__ row, int64_t M, int64_t n_slots,
                                                  UpSel s, int64_t tiles, int nb, uint32_t* __restrict__ part) {
  __shared__ uint32_t h[kUpBins];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long before = (1ull << (threadIdx.x & 63)) - 1ull;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * kUpTile;
    int64_t t[kUpIter];
#pragma unroll
    for (int j = 0; j < kUpIter; j++) t[j] = up_load(next, row, M, n_slots, t0 + j * 256 + threadIdx.x);
#pragma unroll
    for (int j = 0; j < kUpIter; j++) {
      unsigned long long d = 0;
      const bool in = up_class(t[j], s, &d) == kIn;
      const uint32_t bin =
          s.log ? uint32_t(d == 0 ? 0 : 64 - __builtin_clzll(d)) : uint32_t(d >> s.shift) & (kUpBins - 1);
      // Half of a spread table shares the top log bin, and ties share a digit:
      // the lanes of one bin are found by 8 ballots (the multisplit of
      // k_rs_scatter) and their first lane adds their number, so no two lanes
      // of a wave add to one LDS word.
      unsigned long long peers = __ballot(in);
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const bool bit = (bin >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
      }
      if (in && (peers & before) == 0) atomicAdd(&h[bin], uint32_t(__popcll(peers)));
    }
  }
  __syncthreads();
  if (int(threadIdx.x) < nb) part[int64_t(threadIdx.x) * gridDim.x + blockIdx.x] = h[threadIdx.x];  // bin-major
}

// totals[b] = sum of bin b's row of the partial histograms; one block per bin
__global__ __launch_bounds__(256) void k_up_colsum(const uint32_t* __restrict__ part, int G,
                                                    unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long s_sum[4];
  unsigned long long c = 0;
  for (int g = threadIdx.x; g < G; g += 256) c += part[int64_t(blockIdx.x) * G + g];
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) totals[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// candidate j * 256 + wave * 64 + lane of a tile sits in wave word j * 4 + wave
__global__ __launch_bounds__(256) void k_up_count(const int64_t* __restrict__ next,
                                                   const int32_t* __restrict__ row, int64_t M, int64_t n_slots,
                                                   UpSel s, int32_t* __restrict__ cnt_lt,
                                                   int32_t* __restrict__ cnt_cl) {
  __shared__ int32_t s_lt[4], s_cl[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t t0 = int64_t(blockIdx.x) * kUpTile;
  int64_t t[kUpIter];
#pragma unroll
  for (int j = 0; j < kUpIter; j++) t[j] = up_load(next, row, M, n_slots, t0 + j * 256 + threadIdx.x);
  int32_t lt = 0, cl = 0;
#pragma unroll
  for (int j = 0; j < kUpIter; j++) {
    unsigned long long d;
    const int c = up_class(t[j], s, &d);
    lt += __popcll(__ballot(c == kBelow));
    cl += __popcll(__ballot(c == kIn));
  }
  if (lane == 0) {
    s_lt[wv] = lt;
    s_cl[wv] = cl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt_lt[blockIdx.x] = s_lt[0] + s_lt[1] + s_lt[2] + s_lt[3];
    cnt_cl[blockIdx.x] = s_cl[0] + s_cl[1] + s_cl[2] + s_cl[3];
  }
}

// An entry lands behind the BELOW entries before it and the IN entries before
// it that are taken: at below_before + min(in_before, r); an IN entry is taken
// when in_before < r.
__global__ __launch_bounds__(256) void k_up_write(const int64_t* __restrict__ next,
                                                   const int32_t* __restrict__ row, int64_t M, int64_t n_slots,
                                                   UpSel s, const int64_t* __restrict__ base_lt,
                                                   const int64_t* __restrict__ base_cl, int64_t cap,
                                                   unsigned long long* __restrict__ ckey,
                                                   int32_t* __restrict__ cslot) {
  __shared__ int32_t s_lt[kUpWords], s_cl[kUpWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t lt0 = base_lt[blockIdx.x], cl0 = base_cl[blockIdx.x];
  // uniform: nothing of this tile is taken
  if (base_lt[blockIdx.x + 1] == lt0 && (base_cl[blockIdx.x + 1] == cl0 || cl0 >= int64_t(s.r))) return;
  const int64_t t0 = int64_t(blockIdx.x) * kUpTile;
  int64_t t[kUpIter];
#pragma unroll
  for (int j = 0; j < kUpIter; j++) t[j] = up_load(next, row, M, n_slots, t0 + j * 256 + threadIdx.x);
#pragma unroll
  for (int j = 0; j < kUpIter; j++) {
    unsigned long long d;
    const int c = up_class(t[j], s, &d);
    const unsigned long long bl = __ballot(c == kBelow), bi = __ballot(c == kIn);
    if (lane == 0) {
      s_lt[j * 4 + wv] = __popcll(bl);
      s_cl[j * 4 + wv] = __popcll(bi);
    }
  }
  __syncthreads();
  if (wv == 0) {  // exclusive prefix over the tile's 64 words
    const int32_t a = s_lt[lane], b = s_cl[lane];
    int32_t ia = a, ib = b;
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
      if (lane >= o) {
        ia += ua;
        ib += ub;
      }
    }
    s_lt[lane] = ia - a;
    s_cl[lane] = ib - b;
  }
  __syncthreads();
  const unsigned long long before = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kUpIter; j++) {
    unsigned long long d = 0;
    const int c = up_class(t[j], s, &d);
    const unsigned long long bl = __ballot(c == kBelow), bi = __ballot(c == kIn);
    if (c == kNone) continue;
    const int64_t lt = lt0 + s_lt[j * 4 + wv] + __popcll(bl & before);
    const int64_t in = cl0 + s_cl[j * 4 + wv] + __popcll(bi & before);
    if (c == kIn && in >= int64_t(s.r)) continue;
    const int64_t pos = lt + std::min<int64_t>(in, int64_t(s.r));
    if (pos >= cap) continue;  // (the counts of the same table bound it: never taken)
    const int64_t i = t0 + j * 256 + threadIdx.x;
    ckey[pos] = c == kBelow ? (up_key(t[j]) - s.base) : s.lo + d;
    cslot[pos] = row ? row[i] : int32_t(i);
  }
}

// m <= kUpSmall entries: rank of entry i = entries with a smaller (off, i)
__global__ __launch_bounds__(256) void k_up_sort_small(const unsigned long long* __restrict__ ckey,
                                                        const int32_t* __restrict__ cslot, int m, int n_out,
                                                        unsigned long long base,
                                                        const int64_t* __restrict__ prev,
                                                        int32_t* __restrict__ o_slot, int64_t* __restrict__ o_next,
                                                        int64_t* __restrict__ o_prev) {
  __shared__ unsigned long long k[kUpSmall];
  for (int i = threadIdx.x; i < m; i += 256) k[i] = ckey[i];
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += 256) {
    const unsigned long long ki = k[i];
    int rank = 0;
    for (int j = 0; j < m; j++) rank += (k[j] < ki || (k[j] == ki && j < i)) ? 1 : 0;
    if (rank < n_out) {
      const int32_t sl = cslot[i];
      o_slot[rank] = sl;
      o_next[rank] = int64_t((ki + base) ^ kSign);
      o_prev[rank] = prev[sl];
    }
  }
}

// one LSD round's keys: 31 bits of off from `shift` up, of the entry the
// permutation holds at i (val_in null: the identity, written to val_out)
__global__ void k_up_chunk(const unsigned long long* __restrict__ ckey, const int32_t* __restrict__ val_in,
                           int64_t m, int shift, uint32_t* __restrict__ key32, int32_t* __restrict__ val_out) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= m) return;
  const int32_t v = val_in ? val_in[i] : int32_t(i);
  key32[i] = uint32_t(ckey[v] >> shift) & 0x7FFFFFFFu;
  if (!val_in) val_out[i] = v;
}

__global__ void k_up_gather(const unsigned long long* __restrict__ ckey, const int32_t* __restrict__ cslot,
                            const int32_t* __restrict__ val, int64_t n_out, unsigned long long base,
                            const int64_t* __restrict__ prev, int32_t* __restrict__ o_slot,
                            int64_t* __restrict__ o_next, int64_t* __restrict__ o_prev) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n_out) return;
  const int32_t v = val ? val[i] : int32_t(i);
  const int32_t sl = cslot[v];
  o_slot[i] = sl;
  o_next[i] = int64_t((ckey[v] + base) ^ kSign);
  o_prev[i] = prev[sl];
}

int bit_length(unsigned long long x) { return x ? 64 - __builtin_clzll(x) : 0; }

// One histogram pass over the candidates; h[0..nb) on the host.
int up_hist(cg_dispatcher* d, const int32_t* row, int64_t M, const UpSel& s, int nb, unsigned long long* h) {
  cg_ctx* c = d->ctx;
  DispatchUpcoming& u = d->up;
  const int64_t tiles = (M + kUpTile - 1) / kUpTile;
  const int G = int(std::min<int64_t>(tiles, kUpHistBlocks));
  hipLaunchKernelGGL(k_up_hist, dim3(G), dim3(256), 0, c->st, d->next, row, M, d->n, s, tiles, nb, u.part.p);
  hipLaunchKernelGGL(k_up_colsum, dim3(nb), dim3(256), 0, c->st, u.part.p, G, u.totals_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
  for (int b = 0; b < nb; b++) h[b] = u.totals_host[b];
  u.passes++;
  return CG_OK;
}

// the bin of h[0..nb) holding the entry of 1-based rank `want`; *before = the
// entries of the bins below it
int pick_bin(const unsigned long long* h, int nb, unsigned long long want, unsigned long long* before) {
  unsigned long long acc = 0;
  for (int b = 0; b < nb; b++) {
    if (acc + h[b] >= want) {
      *before = acc;
      return b;
    }
    acc += h[b];
  }
  *before = acc;
  return -1;
}

// The select, compaction and sort over M candidates (row: a node's slots).
int up_run(cg_dispatcher* d, const int32_t* row, int64_t M, int64_t k, int64_t until, int64_t* n_out,
           int64_t* n_total) {
  cg_ctx* c = d->ctx;
  DispatchUpcoming& u = d->up;
  hipStream_t st = c->st;
  u.valid = false;
  u.n_out = u.n_total = 0;
  u.passes = 0;
  for (float& m : u.ms) m = 0.f;
  *n_out = *n_total = 0;
  if (M <= 0 || d->effective == CG_ZERO_TIME || until < d->effective) {
    u.valid = true;  // an empty list
    return CG_OK;
  }
  const int64_t tiles = (M + kUpTile - 1) / kUpTile;
  const int64_t hw = radix_hist_words(kUpCap);
  int rc;
  if (!u.totals_host) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&u.totals_host), kUpBins * 8,
                         hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&u.totals_dev), u.totals_host, 0));
  }
  if ((rc = u.part.ensure(size_t(kUpHistBlocks) * kUpBins)) ||
      (rc = u.cnt_lt.ensure(size_t(tiles))) || (rc = u.cnt_cl.ensure(size_t(tiles))) ||
      (rc = u.base_lt.ensure(size_t(tiles) + 1)) || (rc = u.base_cl.ensure(size_t(tiles) + 1)) ||
      (rc = u.ckey.ensure(size_t(kUpCap))) || (rc = u.cslot.ensure(size_t(kUpCap))) ||
      (rc = u.key0.ensure(size_t(kUpCap))) || (rc = u.key1.ensure(size_t(kUpCap))) ||
      (rc = u.val0.ensure(size_t(kUpCap))) || (rc = u.val1.ensure(size_t(kUpCap))) ||
      (rc = u.hist.ensure(size_t(hw))) || (rc = u.hist_off.ensure(size_t(hw) + 1)) ||
      (rc = u.scan_tmp.ensure(std::max(scan_temp_bytes(tiles), scan_temp_bytes(hw)))) ||
      (rc = u.slots.ensure(CG_UPCOMING_MAX)) || (rc = u.next.ensure(CG_UPCOMING_MAX)) ||
      (rc = u.prev.ensure(CG_UPCOMING_MAX)))
    return rc;
  for (hipEvent_t& e : u.ev)
    if (!e) HIPCHK(hipEventCreate(&e));

  // ---- select ----
  (void)hipEventRecord(u.ev[0], st);
  UpSel s{};
  s.base = uint64_t(d->effective) ^ kSign;
  s.uoff = (uint64_t(until) ^ kSign) - s.base;
  s.lo = 0;
  s.w = 64;
  s.log = 1;
  unsigned long long h[kUpBins];
  if ((rc = up_hist(d, row, M, s, kUpLogBins, h))) return rc;
  unsigned long long total = 0;
  int top = 0;  // bit length of the largest off that may be taken
  for (int b = 0; b < kUpLogBins; b++) {
    total += h[b];
    if (h[b]) top = b;
  }
  s.log = 0;
  if (total == 0) {
    u.valid = true;
    return CG_OK;
  }
  unsigned long long m;  // entries the compaction collects
  if (total <= uint64_t(k)) {
    s.r = m = total;  // every firing candidate: all of them IN
  } else {
    // sort a few more than k where that saves a pass over the table
    const unsigned long long stop = std::min<unsigned long long>(kUpCap, std::max<unsigned long long>(2 * k, 2048));
    unsigned long long c_lt = 0;
    const int b = pick_bin(h, kUpLogBins, uint64_t(k), &c_lt);
    if (b < 0) return cg_fail(CG_EHIP, "cg_dispatcher_upcoming: histogram does not hold its own total");
    unsigned long long c_in = h[b];
    top = b;
    s.lo = b ? 1ull << (b - 1) : 0;
    s.w = b ? b - 1 : 0;
    for (;;) {
      if (c_lt + c_in <= stop) {  // take the whole bin
        s.r = c_in;
        m = c_lt + c_in;
        break;
      }
      if (s.w == 0) {  // the k-th key itself: its first ties
        s.r = uint64_t(k) - c_lt;
        m = uint64_t(k);
        break;
      }
      s.shift = std::max(s.w - 8, 0);
      const int nb = 1 << (s.w - s.shift);
      if ((rc = up_hist(d, row, M, s, nb, h))) return rc;
      unsigned long long before = 0;
      const int dg = pick_bin(h, nb, uint64_t(k) - c_lt, &before);
      if (dg < 0) return cg_fail(CG_EHIP, "cg_dispatcher_upcoming: histogram does not hold its own total");
      c_lt += before;
      c_in = h[dg];
      s.lo += uint64_t(dg) << s.shift;
      s.w = s.shift;
    }
  }
  const int64_t out = int64_t(std::min<unsigned long long>(total, uint64_t(k)));
  if (m > uint64_t(kUpCap) || uint64_t(out) > m)
    return cg_fail(CG_EHIP, "cg_dispatcher_upcoming: the select took " + std::to_string(m) + " entries");

  // ---- compaction, ascending in candidate order ----
  (void)hipEventRecord(u.ev[1], st);
  hipLaunchKernelGGL(k_up_count, dim3(unsigned(tiles)), dim3(256), 0, st, d->next, row, M, d->n, s, u.cnt_lt.p,
                     u.cnt_cl.p);
  launch_scan(u.cnt_lt.p, u.base_lt.p, tiles, u.scan_tmp.p, st);
  launch_scan(u.cnt_cl.p, u.base_cl.p, tiles, u.scan_tmp.p, st);
  hipLaunchKernelGGL(k_up_write, dim3(unsigned(tiles)), dim3(256), 0, st, d->next, row, M, d->n, s, u.base_lt.p,
                     u.base_cl.p, kUpCap, u.ckey.p, u.cslot.p);
  u.passes += 2;
  HIPCHK(hipGetLastError());

  // ---- sort by (off, candidate order), gather ----
  (void)hipEventRecord(u.ev[2], st);
  if (int64_t(m) <= kUpSmall) {
    hipLaunchKernelGGL(k_up_sort_small, dim3(1), dim3(256), 0, st, u.ckey.p, u.cslot.p, int(m), int(out), s.base,
                       d->prev, u.slots.p, u.next.p, u.prev.p);
  } else {
    const int32_t* perm = nullptr;
    uint32_t* k0 = reinterpret_cast<uint32_t*>(u.key0.p);
    uint32_t* k1 = reinterpret_cast<uint32_t*>(u.key1.p);
    int32_t *v0 = u.val0.p, *v1 = u.val1.p;
    const unsigned grid = unsigned((m + 255) / 256);
    for (int shift = 0; shift < top; shift += 31) {
      hipLaunchKernelGGL(k_up_chunk, dim3(grid), dim3(256), 0, st, u.ckey.p, perm, int64_t(m), shift, k0, v0);
      const int bits = std::min(top - shift, 31);
      bool in_second = false;
      radix_by_key_enqueue(st, k0, v0, k1, v1, int64_t(m), bits >= 31 ? INT32_MAX : int32_t(1) << bits,
                           u.hist.p, u.hist_off.p, u.scan_tmp.p, &in_second);
      if (in_second) {
        std::swap(k0, k1);
        std::swap(v0, v1);
      }
      perm = v0;
      // the next round reads the permutation from v0 and writes its keys to
      // k0; its first scatter then fills (k1, v1)
    }
    hipLaunchKernelGGL(k_up_gather, dim3(unsigned((out + 255) / 256)), dim3(256), 0, st, u.ckey.p, u.cslot.p, perm,
                       out, s.base, d->prev, u.slots.p, u.next.p, u.prev.p);
  }
  (void)hipEventRecord(u.ev[3], st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < DispatchUpcoming::kPhases; i++) (void)hipEventElapsedTime(&u.ms[i], u.ev[i], u.ev[i + 1]);
  u.n_out = out;
  u.n_total = int64_t(total);
  u.valid = true;
  *n_out = u.n_out;
  *n_total = u.n_total;
  return CG_OK;
}

int up_check(cg_dispatcher* d, int64_t k, int64_t* n_out, int64_t* n_total, const char* who) {
  if (!d || !n_out || !n_total) return cg_fail(CG_EINVAL, std::string(who) + ": null");
  if (k < 1 || k > CG_UPCOMING_MAX)
    return cg_fail(CG_EINVAL, std::string(who) + ": k outside [1, " + std::to_string(CG_UPCOMING_MAX) + "]");
  return CG_OK;
}

int up_pending(cg_ctx* c) {
  if (pn_async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined per-node windows pending (call cg_expand_per_node_wait first)");
  if (async_pending(c))
    return cg_fail(CG_EINVAL, "pipelined rule-major calls pending (call cg_expand_wait first)");
  return CG_OK;
}

}  // namespace

extern "C" {

int cg_dispatcher_upcoming(cg_dispatcher* d, int64_t k, int64_t until, int64_t* n_out, int64_t* n_total) {
  int rc = up_check(d, k, n_out, n_total, "cg_dispatcher_upcoming");
  if (rc) return rc;
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  if ((rc = up_pending(c))) return rc;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  return up_run(d, nullptr, d->n, k, until, n_out, n_total);
}

int cg_dispatcher_upcoming_node(cg_dispatcher* d, int32_t node, int64_t k, int64_t until, int64_t* n_out,
                                int64_t* n_total) {
  int rc = up_check(d, k, n_out, n_total, "cg_dispatcher_upcoming_node");
  if (rc) return rc;
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  const DispatchFanout& f = d->fo;
  if (!f.bound)
    return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_node: no rule set bound (cg_dispatcher_bind_rules)");
  if (node < 0 || node >= f.N)
    return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_node: node " + std::to_string(node) + " outside the bound " +
                                  std::to_string(f.N) + " nodes");
  if ((rc = up_pending(c))) return rc;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  int64_t lohi[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(lohi, f.nt_off.p + node, 16, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (lohi[0] < 0 || lohi[1] < lohi[0] || lohi[1] > f.nnz)
    return cg_fail(CG_EHIP, "cg_dispatcher_upcoming_node: the bound join's node offsets are out of order");
  return up_run(d, f.nt_rule.p + lohi[0], lohi[1] - lohi[0], k, until, n_out, n_total);
}

int cg_dispatcher_upcoming_copy(const cg_dispatcher* d, int32_t* slots, int64_t* next, int64_t* prev,
                                int64_t cap) {
  if (!d) return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_copy: null");
  cg_ctx* c = d->ctx;
  std::lock_guard<std::mutex> g(c->mu);
  const DispatchUpcoming& u = d->up;
  if (!u.valid)
    return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_copy: no list since the last set / remove / fire / "
                              "patch / bind");
  if ((slots || next || prev) && cap < u.n_out)
    return cg_fail(CG_ECAPACITY, "cg_dispatcher_upcoming_copy: buffers too small, " + std::to_string(u.n_out) +
                                     " entries required");
  if (!u.n_out) return CG_OK;
  (void)hipGetLastError();
  HIPCHK(hipSetDevice(c->device));
  const size_t n = size_t(u.n_out);
  if (slots) HIPCHK(hipMemcpyAsync(slots, u.slots.p, n * 4, hipMemcpyDeviceToHost, c->st));
  if (next) HIPCHK(hipMemcpyAsync(next, u.next.p, n * 8, hipMemcpyDeviceToHost, c->st));
  if (prev) HIPCHK(hipMemcpyAsync(prev, u.prev.p, n * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return CG_OK;
}

int cg_dispatcher_upcoming_device(const cg_dispatcher* d, const int32_t** d_slots, const int64_t** d_next,
                                  const int64_t** d_prev, int64_t* n) {
  if (!d) return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_device: null");
  std::lock_guard<std::mutex> g(d->ctx->mu);
  const DispatchUpcoming& u = d->up;
  if (!u.valid)
    return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_device: no list since the last set / remove / fire / "
                              "patch / bind");
  if (d_slots) *d_slots = u.slots.p;
  if (d_next) *d_next = u.next.p;
  if (d_prev) *d_prev = u.prev.p;
  if (n) *n = u.n_out;
  return CG_OK;
}

int cg_dispatcher_upcoming_times(const cg_dispatcher* d, float* ms, int n) {
  if (!d || !ms || n < 0) return cg_fail(CG_EINVAL, "cg_dispatcher_upcoming_times: null");
  std::lock_guard<std::mutex> g(d->ctx->mu);
  const DispatchUpcoming& u = d->up;
  const float v[DispatchUpcoming::kPhases + 1] = {u.ms[0], u.ms[1], u.ms[2], float(u.passes)};
  const int k = std::min(n, DispatchUpcoming::kPhases + 1);
  for (int i = 0; i < k; i++) ms[i] = v[i];
  return k;
}

}  // extern "C"
