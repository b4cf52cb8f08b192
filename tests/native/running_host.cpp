// Host-side check of the running profile algorithm, in both flavours: the
// shared CG_HD routines a RUNNING call runs -- the in-flight base rows
// (inflight_cell, inflight_walk_row as k_inflight_rules / k_inflight_walk leave
// them), admit_walk_unit / lock_walk_unit with the difference emit
// (cg_profile.h, running_emit_diff) into the zeroed rows, then a host row scan
// standing in for k_rows_prefix -- against the literal process of the
// definition over the oracle's Next loop: the fires that start (admit_host.cpp's
// and lock_host.cpp's fire-by-fire passes, the latter with the oracle's
// or_lock_ttl at now = t), counted at every bucket edge e while
// a <= e and a * 1000 + ms > e * 1000.
// Zones, specs, t0 choices, shapes and unit sizes are admit_host.cpp's; the
// admission flavour runs its P values and durations, the lock flavour
// lock_host.cpp's kinds, avg_ms, lock_ttl cycle and non-contending rules, over
// the zone table a lock profile stages.
// Test infrastructure; the GPU tests check the kernels themselves.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <random>
#include <unordered_map>

#include "../../cronsun_amd/csrc/cg_lock.h"
#include "host_common.h"

using namespace cg;

static const char* atoms[6][16] = {
    {"*/7", "0", "5", "*/20", "15/35", "10-40/3", "7,30,45", "59", "0/15", "3-3", "0", "58-59", "0", "0", "30", "*/30"},
    {"*", "0", "30", "*/5", "20-35/15", "1,31,59", "5-7/2", "*/59", "10-12", "0", "0", "59", "45", "15", "0,30", "*/15"},
    {"*", "0", "9", "23", "*/2", "1/2", "9-17", "22,23,0", "2", "1", "3", "0-23/5", "0", "1", "0,1", "23"},
    {"*", "?", "1", "15", "31", "29", "30", "1,15", "*/2", "9-20", "28-31", "5/7", "8", "*", "?", "1-7"},
    {"*", "?", "1", "2", "Feb", "Jan,Jul", "Apr-Oct", "*/3", "Mar", "Nov", "Dec", "*", "*", "*", "Oct", "Sep-Dec"},
    {"*", "?", "0", "1-5", "Mon", "Sun", "mon/2", "Sat,Sun", "*/2", "3", "fri-sat", "*", "*", "0", "6", "?"}};
static const char* specials[] = {"* * * * * *", "@every 11s", "@every 5400s", "@every 360000s", "0 0 0 30 Feb ?",
                                 "7,30,45 * * * * *", "0 30 2 * * *", "@daily"};

struct Shape {
  int64_t w;
  int32_t B;
};
static const Shape shapes[] = {{1, 130}, {7, 1000}, {37, 1200}, {60, 65}, {1800, 24}, {3600, 48}, {86400, 3}, {604800, 14}};
static const int64_t avgs[] = {0, 999, 1000, 2500, 60000, 3600000, -1500, INT64_MAX};
static const int64_t ttls[] = {2, 300, 600};

// is a command started at a with a run time of ms still running at t >= a?
static bool running(int64_t a, int64_t ms, int64_t t) {
  return ms / 1000 > t - a || (ms / 1000 == t - a && ms % 1000 != 0);  // a * 1000 + ms > t * 1000
}

// The literal count of one rule: its started fires (ascending) in flight at
// every edge.  Started fires end in start order (one ms per row), so those in
// flight at an edge are a window of the list: both ends only move forward.
static void literal_row(const std::vector<int64_t>& started, int64_t ms, int64_t t0, int64_t w, int32_t B, int32_t* row) {
  size_t head = 0, tail = 0;
  for (int32_t b = 0; b < B; b++) {
    const int64_t e = t0 + (int64_t(b) + 1) * w;
    while (head < started.size() && started[head] <= e) head++;
    while (tail < head && !running(started[tail], ms, e)) tail++;
    row[b] = int32_t(head - tail);
  }
}

// the rules of one horizon under one plan: specs, run records at stride G, and
// the in-flight base rows per (rule, d), computed when first asked for
struct Recs {
  Plan plan;
  ZoneView zv;
  int G = 0;
  int64_t t0 = 0, t1 = 0, w = 0;
  int32_t B = 0;
  std::vector<DSpec> specs;
  std::vector<size_t> src;  // index into the horizon's spec list
  std::vector<int64_t> anc;
  std::vector<int32_t> cnt;
  std::vector<uint32_t> dm;
  std::map<std::pair<int64_t, int64_t>, std::vector<int32_t>> base;
  long long walked_fires = 0;

  const std::vector<int32_t>& inflight_row(int64_t r, int64_t d) {
    auto it = base.find({r, d});
    if (it != base.end()) return it->second;
    std::vector<int32_t> row(size_t(B), 0);
    const CFRule c = cf_rule(specs[r]);
    const size_t j0 = size_t(r) * G;
    for (int32_t b = 0; b < B; b++)  // k_inflight_rules
      row[b] = inflight_cell(specs[r], c, plan.segs.data(), G, anc.data() + j0, cnt.data() + j0, dm.data() + j0, t0, t1,
                             t0 + (int64_t(b) + 1) * w, d);
    inflight_walk_row(specs[r], zv, plan.segs.data(), G, anc.data() + j0, cnt.data() + j0, dm.data() + j0, t0, t1, w, B, d,
                      row.data());  // k_inflight_walk
    return base.emplace(std::make_pair(r, d), std::move(row)).first->second;
  }
};

// k_rows_prefix on the host: an inclusive prefix sum along the row
static void row_scan(int32_t* row, int32_t B) {
  for (int32_t b = 1; b < B; b++) row[b] += row[b - 1];
}

int main(int argc, char** argv) {
  const char* zone = argc > 1 ? argv[1] : "UTC";
  const int nspec = argc > 2 ? atoi(argv[2]) : 60;
  const long long budget = argc > 4 ? atoll(argv[4]) : 300000;
  const int64_t kRuleCap = std::min<long long>(200000, budget);
  std::vector<int64_t> buf(kRuleCap);
  ZoneRules zr;
  or_loc* ol = nullptr;
  load_zone(zone, &zr, &ol);
  std::mt19937_64 rng(argc > 3 ? strtoull(argv[3], nullptr, 10) : 777);
  std::vector<or_sched> scheds;
  std::vector<std::string> names;
  size_t nspecial = 0;
  while ((int)scheds.size() < nspec) {
    std::string spec;
    if (nspecial < sizeof specials / sizeof specials[0]) spec = specials[nspecial++];
    else if (rng() % 10 == 0) spec = "@every " + std::to_string(1 + rng() % 7200) + "s";
    else for (int f = 0; f < 6; f++) { if (f) spec += " "; spec += atoms[f][rng() % 16]; }
    or_sched s;
    char err[256];
    if (or_parse(OR_OPT_DEFAULT, spec.c_str(), spec.size(), &s, err, sizeof err)) continue;
    scheds.push_back(s);
    names.push_back(spec);
  }
  std::vector<int64_t> t0s = {1767571217};  // 2026-01-05 00:00:17 UTC
  ZoneTable tt = build_table(zr, 1767225600, 1798761600);
  for (size_t i = 1; i < tt.when.size() && i < 3; i++) {
    t0s.push_back(tt.when[i] - 6 * 3600 + 17);
    if (i == 1) t0s.push_back(tt.when[i] - 1801);
  }
  int bad = 0, skipped_h = 0, horizons = 0;
  long long total = 0, cells = 0, walked_fires = 0, admit_walks = 0, plain_units = 0, dropped_all = 0, lock_walks = 0,
            granted_all = 0, skipped_all = 0, stuck_walks = 0, diff_fires = 0, below_inflight = 0;
  unsigned combo = 0;
  for (int64_t t0 : t0s)
    for (const Shape& sh : shapes) {
      const int64_t w = sh.w, t1 = t0 + sh.B * w;
      const int32_t B = sh.B;
      horizons++;
      std::vector<std::vector<int64_t>> exp(scheds.size());
      std::vector<char> use(scheds.size(), 0);
      long long ev = 0;
      bool stuck = false;
      for (size_t r = 0; r < scheds.size() && !stuck && ev <= budget; r++) {
        const int64_t h1 = t1 - t0 < 86400 ? t1 - t0 : 86400;
        const int64_t n1 = or_expand(&scheds[r], t0, t0 + h1, ol, nullptr, 0);
        if (n1 >= 0 && n1 * ((t1 - t0) / h1) > kRuleCap) continue;
        const int64_t n = or_expand(&scheds[r], t0, t1, ol, buf.data(), kRuleCap);
        if (n < 0) { stuck = true; break; }
        if (n > kRuleCap) continue;
        exp[r].assign(buf.begin(), buf.begin() + n);
        use[r] = 1;
        ev += n;
      }
      if (stuck) { skipped_h++; continue; }
      total += ev;
      // the used rules under the horizon's own plan (admission) and under the
      // plan with the lock profile's longer zone table (lock)
      Recs recs[2];
      for (int lock = 0; lock < 2; lock++) {
        Recs& rc = recs[lock];
        rc.plan = build_plan(zr, t0, t1);
        if (lock) rc.plan.table = build_lock_table(zr, t0, t1);  // as run_set_count_scan stages it
        rc.zv = ZoneView{rc.plan.table.when.data(), rc.plan.table.off.data(), int32_t(rc.plan.table.when.size())};
        rc.G = int(rc.plan.segs.size());
        rc.t0 = t0, rc.t1 = t1, rc.w = w, rc.B = B;
        const int G = rc.G;
        for (size_t r = 0; r < exp.size(); r++) {
          if (!use[r]) continue;
          const DSpec d = pack(scheds[r]);
          const size_t j0 = rc.specs.size() * size_t(G);
          rc.anc.resize(j0 + G);
          rc.cnt.resize(j0 + G);
          rc.dm.resize(j0 + G);
          const bool ok = count_rule(d, rc.zv, rc.plan.segs.data(), G, rc.plan.dtab.data(), t0, t1, rc.plan.flags,
                                     rc.anc.data() + j0, rc.cnt.data() + j0, rc.dm.data() + j0);
          if (!ok) {
            if (bad++ < 10) printf("STUCK mismatch %s [%s] t0=%lld w=%lld B=%d\n", zone, names[r].c_str(), (long long)t0, (long long)w, B);
            rc.anc.resize(j0);
            rc.cnt.resize(j0);
            rc.dm.resize(j0);
            continue;
          }
          for (int s = 0; s < G; s++)
            if (rc.cnt[j0 + s] && !run_has_closed_form(d, rc.plan.segs[s], rc.dm[j0 + s])) rc.walked_fires += rc.cnt[j0 + s];
          rc.specs.push_back(d);
          rc.src.push_back(r);
        }
      }
      if (recs[0].src != recs[1].src) {
        if (bad++ < 10) printf("PLAN mismatch %s t0=%lld w=%lld B=%d: the two plans keep different rules\n", zone, (long long)t0, (long long)w, B);
        continue;
      }
      walked_fires += recs[0].walked_fires;
      const int64_t R = int64_t(recs[0].specs.size());
      const std::vector<size_t>& src = recs[0].src;
      const int64_t durs[] = {0, 1, 999, 1000, 1001, w * 1000 - 1, w * 1000, w * 1000 + 1, 3500 * w,
                              45LL * 86400 * 1000, INT64_MAX};
      std::unordered_map<uint64_t, int64_t> memo;
      auto oracle_ttl = [&](size_t rule, int64_t t, int kind, int ai, int li) {
        const uint64_t key = (uint64_t(t - t0) << 16) | (uint64_t(rule) << 8) | uint64_t(kind << 5 | ai << 2 | li);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        const int64_t v = or_lock_ttl(&scheds[rule], t, 0, ol, kind, avgs[ai], ttls[li]);
        memo.emplace(key, v);
        return v;
      };
      // compares one unit's rows, counts the cells and those below the in-flight rows
      auto compare = [&](Recs& rc, const char* flavour, int64_t r0, int64_t k, int64_t d, const std::vector<int32_t>& got,
                         const std::vector<int32_t>& want, long long a, long long b2, long long c) {
        cells += k * B;
        for (int64_t r = r0; r < r0 + k; r++) {
          const std::vector<int32_t>& infl = rc.inflight_row(r, d);
          for (int32_t b = 0; b < B; b++) {
            const int32_t x = got[(r - r0) * B + b];
            if (x > infl[b] && bad++ < 10)
              printf("ABOVE IN-FLIGHT %s %s rule +%lld bucket %d: %d > %d\n", flavour, zone, (long long)(r - r0), b, x, infl[b]);
            if (x < infl[b]) below_inflight++;
          }
        }
        if (got != want && bad++ < 10) {
          size_t i = 0;
          while (got[i] == want[i]) i++;
          printf("MISMATCH %s %s unit [%s..] k=%lld t0=%lld w=%lld B=%d (%lld, %lld, %lld) rule +%zu bucket %zu: %d vs %d (G=%d)\n",
                 flavour, zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, B, a, b2, c, i / B, i % B,
                 got[i], want[i], rc.G);
        }
      };
      for (int usz : {1, 2, 5, kAdmitWalkSlots + 1})  // the last: two rules share a remembered position
        for (int64_t r0 = 0; r0 < R; r0 += usz) {
          const int64_t k = std::min<int64_t>(usz, R - r0);
          // ---------------------------------------------- admission flavour --
          {
            Recs& rc = recs[0];
            std::vector<std::pair<int64_t, int32_t>> fires;
            for (int64_t r = r0; r < r0 + k; r++)
              for (int64_t t : exp[src[r]]) fires.push_back({t, int32_t(r - r0)});
            std::sort(fires.begin(), fires.end());
            for (int64_t P : {0, 1, 2, 16})
              for (int64_t ms : durs) {
                // the literal process: which fires start
                std::vector<std::vector<int64_t>> started(static_cast<size_t>(k));
                std::vector<int64_t> admitted;
                for (const auto& f : fires) {
                  int64_t busy = 0;
                  for (size_t i = admitted.size(); busy < P && i-- > 0 && running(admitted[i], ms, f.first);) busy++;
                  if (P == 0 || busy < P) {
                    admitted.push_back(f.first);
                    started[size_t(f.second)].push_back(f.first);
                  } else {
                    dropped_all++;
                  }
                }
                std::vector<int32_t> want(size_t(k) * B, 0);
                for (int64_t i = 0; i < k; i++) literal_row(started[size_t(i)], ms, t0, w, B, want.data() + i * B);
                // the engine's way
                const int64_t d = inflight_seconds(ms, int64_t(B) * w);
                std::vector<int32_t> got(size_t(k) * B, 0);
                if (!admit_never_drops(P, d, k)) {
                  admit_walks++;  // k_admit_prepare zeroed the rows
                  int64_t ring[kAdmitMaxParallels], wt[kAdmitWalkSlots];
                  int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                  const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                  const AdmitUnit u{r0, d, int32_t(k), int32_t(P)};
                  admit_walk_unit(rc.specs.data(), rc.zv, rc.plan.segs.data(), rc.G, rc.anc.data(), rc.cnt.data(),
                                  rc.dm.data(), t0, t1, u, ring, 1, wc, [&](int64_t r, int64_t t) {
                                    if (t <= t0 || t > t1 || r < r0 || r >= r0 + k) { bad++; return; }
                                    diff_fires++;
                                    running_emit_diff(got.data() + (r - r0) * B, B, t, u.d, t0, w);
                                  });
                  for (int64_t i = 0; i < k; i++) row_scan(got.data() + i * B, B);
                } else {
                  plain_units++;
                  for (int64_t i = 0; i < k; i++) {
                    const std::vector<int32_t>& row = rc.inflight_row(r0 + i, d);
                    std::copy(row.begin(), row.end(), got.begin() + i * B);
                  }
                }
                compare(rc, "admission", r0, k, d, got, want, (long long)P, (long long)ms, 0);
              }
          }
          // --------------------------------------------------- lock flavour --
          Recs& rc = recs[1];
          for (int kind : {JOB_ALONE, JOB_INTERVAL})
            for (int ai = 0; ai < int(sizeof avgs / sizeof avgs[0]); ai++) {
              const int64_t avg = avgs[ai], ms = avg > 0 ? avg : 0;
              const int li = (horizons + ai + kind) % 3;
              const int64_t lock_ttl = ttls[li];
              const int hole = int(combo % 4);  // 0: all contend; 1, 2, 3: not the first, middle, last rule
              combo++;
              std::vector<uint8_t> cont(size_t(R), 1);
              if (hole) cont[size_t(r0 + (hole == 1 ? 0 : hole == 2 ? k / 2 : k - 1))] = 0;
              std::vector<std::pair<int64_t, int32_t>> fires;
              std::vector<std::vector<int64_t>> started(static_cast<size_t>(k));
              for (int64_t r = r0; r < r0 + k; r++) {
                if (cont[size_t(r)])
                  for (int64_t t : exp[src[r]]) fires.push_back({t, int32_t(r - r0)});
                else
                  started[size_t(r - r0)] = exp[src[r]];  // reaches no lock: every fire runs
              }
              std::sort(fires.begin(), fires.end());
              bool have_free = false;
              int64_t free_s = 0, free_ms = 0;  // the lease ends at free_s * 1000 + free_ms (no overflow at INT64_MAX ms)
              int64_t want_stuck = -1;
              for (const auto& f : fires) {
                if (have_free && (f.first - free_s < free_ms / 1000 || (f.first - free_s == free_ms / 1000 && free_ms % 1000 != 0))) {
                  skipped_all++;
                  continue;
                }
                const int64_t ttl = oracle_ttl(src[r0 + f.second], f.first, kind, ai, li);
                if (ttl == OR_NO_PROGRESS) { want_stuck = r0 + f.second; break; }
                if (ttl == 0) { skipped_all++; continue; }
                started[size_t(f.second)].push_back(f.first);
                granted_all++;
                have_free = true;
                free_s = f.first + ttl;
                free_ms = kind == JOB_ALONE ? ms : 0;
              }
              std::vector<int32_t> want(size_t(k) * B, 0);
              for (int64_t i = 0; i < k; i++) literal_row(started[size_t(i)], ms, t0, w, B, want.data() + i * B);
              // the engine's way: in-flight rows, the contending rows zeroed and rewritten
              const int64_t d = inflight_seconds(ms, int64_t(B) * w);
              std::vector<int32_t> got(size_t(k) * B, 0);
              bool any = false;
              for (int64_t i = 0; i < k; i++) {
                if (cont[size_t(r0 + i)]) { any = true; continue; }
                const std::vector<int32_t>& row = rc.inflight_row(r0 + i, d);
                std::copy(row.begin(), row.end(), got.begin() + i * B);
              }
              int64_t got_stuck = -1;
              if (any) {
                lock_walks++;
                int64_t wt[kAdmitWalkSlots];
                int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                const LockUnit u{r0, avg, d, int32_t(k), kind};
                got_stuck = lock_walk_unit(rc.specs.data(), rc.zv, rc.plan.segs.data(), rc.G, rc.anc.data(), rc.cnt.data(),
                                           rc.dm.data(), t0, t1, u, lock_ttl, cont.data(), wc, [&](int64_t r, int64_t t) {
                                             if (t <= t0 || t > t1 || r < r0 || r >= r0 + k || !cont[size_t(r)]) { bad++; return; }
                                             diff_fires++;
                                             running_emit_diff(got.data() + (r - r0) * B, B, t, u.d, t0, w);
                                           });
                for (int64_t i = 0; i < k; i++)
                  if (cont[size_t(r0 + i)]) row_scan(got.data() + i * B, B);
              }
              if (got_stuck != want_stuck) {
                if (bad++ < 10)
                  printf("STUCK rule %lld vs %lld: %s unit [%s..] k=%lld t0=%lld w=%lld B=%d\n", (long long)got_stuck,
                         (long long)want_stuck, zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, B);
                continue;
              }
              if (want_stuck >= 0) { stuck_walks++; continue; }  // the rows are unfinished on both sides
              compare(rc, "lock", r0, k, d, got, want, kind, (long long)avg, (long long)lock_ttl);
            }
        }
    }
  printf("%s: %d of %d horizons skipped (non-terminating reference loop)\n", zone, skipped_h, horizons);
  if (4 * skipped_h > horizons) {
    printf("%s: more than a quarter of the horizons skipped\n", zone);
    bad++;
  }
  printf("%s: %d mismatches, %lld cells, %lld events checked, %lld of them walked; %lld admission walks, %lld units that "
         "never drop, %lld fires dropped, %lld lock walks, %lld fires granted, %lld fires skipped, %lld stuck walks, %lld "
         "differences written, %lld cells below in flight\n",
         zone, bad, cells, total, walked_fires, admit_walks, plain_units, dropped_all, lock_walks, granted_all, skipped_all,
         stuck_walks, diff_fires, below_inflight);
  or_loc_free(ol);
  return bad ? 1 : 0;
}
