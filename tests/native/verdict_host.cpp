// Host-side check of the fire verdicts (cg_verdict.h: fire_position over the run
// records of count_rule and their prefix sum, the closed-form rank and the
// search of a walked run's stretch; cg_admit.h / cg_lock.h: the two unit walks
// with the emit that clears a bit at fire_position -- exactly what
// k_admit_verdicts and k_lock_verdicts run, over the zone table a lock call
// stages) against the literal processes of the definition run fire by fire
// over the oracle's Next loop and the oracle's or_lock_ttl at now = t.
//   1. times = the oracle's fire lists, rule-major; run_off = the prefix sum of
//      the run counts.  For every fire of every rule: fire_position == its index.
//   2. admission: units of 1, 2, 5 and 9 rules, P in {0, 1, 2, 16},
//      admit_host.cpp's durations: the bytes after the init and the walk equal
//      the literal process's.
//   3. lock: the same units, both lock kinds, lock_host.cpp's AvgTimes, LockTtls
//      and non-contending holes.
// Zones, specs, t0 choices and shapes are admit_host.cpp's.
// Test infrastructure; the GPU tests check the kernels themselves.
#include <algorithm>
#include <cstdlib>
#include <random>
#include <unordered_map>

#include "../../cronsun_amd/csrc/cg_lock.h"
#include "../../cronsun_amd/csrc/cg_verdict.h"
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

struct Fire {
  int64_t t;
  int64_t rule;  // index among the horizon's used rules
  int64_t pos;   // index in times
  bool operator<(const Fire& o) const { return t != o.t ? t < o.t : rule < o.rule; }
};

int main(int argc, char** argv) {
  const char* zone = argc > 1 ? argv[1] : "UTC";
  const int nspec = argc > 2 ? atoi(argv[2]) : 60;
  // as admit_host.cpp: a rule is checked on a horizon only where it fires at
  // most kRuleCap times there, a horizon's spec list is cut at `budget` fires
  const long long budget = argc > 4 ? atoll(argv[4]) : 100000;
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
  long long positions = 0, walked_positions = 0, admit_walks = 0, dropped_all = 0, lock_walks = 0, skipped_all = 0,
            stuck_walks = 0, bytes = 0;
  unsigned combo = 0;
  for (int64_t t0 : t0s)
    for (const Shape& sh : shapes) {
      const int64_t w = sh.w, t1 = t0 + sh.B * w;
      const int64_t durs[] = {0, 1, 999, 1000, 1001, w * 1000 - 1, w * 1000, w * 1000 + 1, 3500 * w,
                              45LL * 86400 * 1000, INT64_MAX};
      horizons++;
      Plan plan = build_plan(zr, t0, t1);
      plan.table = build_lock_table(zr, t0, t1);  // as a lock call's count chain stages it
      ZoneView zv{plan.table.when.data(), plan.table.off.data(), int32_t(plan.table.when.size())};
      const int G = int(plan.segs.size());
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
      // the used rules, compacted: specs, run records at stride G, the CSR
      std::vector<DSpec> specs;
      std::vector<size_t> src;
      std::vector<int64_t> anc, times, off(1, 0);
      std::vector<int32_t> cnt;
      std::vector<uint32_t> dm;
      for (size_t r = 0; r < exp.size(); r++) {
        if (!use[r]) continue;
        const DSpec d = pack(scheds[r]);
        const size_t j0 = specs.size() * size_t(G);
        anc.resize(j0 + G);
        cnt.resize(j0 + G);
        dm.resize(j0 + G);
        const bool ok = count_rule(d, zv, plan.segs.data(), G, plan.dtab.data(), t0, t1, plan.flags, anc.data() + j0,
                                   cnt.data() + j0, dm.data() + j0);
        if (!ok) {
          if (bad++ < 10) printf("STUCK mismatch %s [%s] t0=%lld w=%lld B=%d\n", zone, names[r].c_str(), (long long)t0, (long long)w, sh.B);
          anc.resize(j0);
          cnt.resize(j0);
          dm.resize(j0);
          continue;
        }
        specs.push_back(d);
        src.push_back(r);
        times.insert(times.end(), exp[r].begin(), exp[r].end());
        off.push_back(int64_t(times.size()));
      }
      const int64_t R = int64_t(specs.size()), E = int64_t(times.size());
      // the scan: run_off[j] = fires of the runs before j, run_off[R * G] = E
      std::vector<int64_t> run_off(size_t(R) * G + 1, 0);
      for (size_t j = 0; j < size_t(R) * G; j++) run_off[j + 1] = run_off[j] + cnt[j];
      if (run_off[size_t(R) * G] != E) {
        if (bad++ < 10) printf("COUNT mismatch %s t0=%lld w=%lld: runs hold %lld fires, the oracle %lld\n", zone, (long long)t0,
                               (long long)w, (long long)run_off[size_t(R) * G], (long long)E);
        continue;
      }
      // 1. every fire's position
      for (int64_t r = 0; r < R; r++) {
        const size_t j0 = size_t(r) * G;
        for (int64_t e = off[r]; e < off[r + 1]; e++) {
          const int64_t p = fire_position(specs[r], plan.segs.data(), G, anc.data() + j0, cnt.data() + j0, dm.data() + j0,
                                          run_off.data() + j0, times.data(), t1, times[e]);
          positions++;
          const int s = seg_after(plan.segs.data(), G, times[e] - 1);
          if (s < G && !run_has_closed_form(specs[r], plan.segs[s], dm[j0 + s])) walked_positions++;
          if (p != e && bad++ < 10)
            printf("POSITION %s [%s] t0=%lld w=%lld B=%d rule %lld fire %lld (t=%lld): %lld vs %lld (G=%d)\n", zone,
                   names[src[r]].c_str(), (long long)t0, (long long)w, sh.B, (long long)r, (long long)(e - off[r]),
                   (long long)times[e], (long long)p, (long long)e, G);
        }
      }
      // the clearing emit of both walks, with the kernels' self-check
      std::vector<uint8_t> got(size_t(E), 0), want(size_t(E), 0);
      auto clear = [&](int64_t r, int64_t t, uint8_t bit) {
        const size_t j0 = size_t(r) * G;
        const int64_t p = fire_position(specs[r], plan.segs.data(), G, anc.data() + j0, cnt.data() + j0, dm.data() + j0,
                                        run_off.data() + j0, times.data(), t1, t);
        if (p < 0 || p >= E || times[p] != t) { bad++; return; }
        got[size_t(p)] &= uint8_t(~bit);
      };
      auto compare = [&](int64_t r0, int64_t k, const char* what, long long a, long long b, long long c) {
        bytes += off[r0 + k] - off[r0];
        for (int64_t e = off[r0]; e < off[r0 + k]; e++)
          if (got[size_t(e)] != want[size_t(e)]) {
            if (bad++ < 10) {
              const int64_t r = std::upper_bound(off.begin(), off.end(), e) - off.begin() - 1;
              printf("MISMATCH %s %s unit [%s..] k=%lld t0=%lld w=%lld B=%d (%lld, %lld, %lld) rule +%lld fire %lld (t=%lld): "
                     "%d vs %d (G=%d)\n",
                     zone, what, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, sh.B, a, b, c,
                     (long long)(r - r0), (long long)(e - off[r]), (long long)times[e], got[e], want[e], G);
            }
            return;
          }
      };
      std::unordered_map<uint64_t, int64_t> memo;  // or_lock_ttl's answers, kept for the horizon (lock_host.cpp)
      auto oracle_ttl = [&](size_t rule, int64_t t, int kind, int ai, int li) {
        const uint64_t key = (uint64_t(t - t0) << 16) | (uint64_t(rule) << 8) | uint64_t(kind << 5 | ai << 2 | li);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        const int64_t v = or_lock_ttl(&scheds[rule], t, 0, ol, kind, avgs[ai], ttls[li]);
        memo.emplace(key, v);
        return v;
      };
      for (int usz : {1, 2, 5, kAdmitWalkSlots + 1})  // the last: two rules share a remembered position
        for (int64_t r0 = 0; r0 < R; r0 += usz) {
          const int64_t k = std::min<int64_t>(usz, R - r0);
          std::vector<Fire> all;  // the unit's fires in (time, rule) order, from the oracle
          for (int64_t r = r0; r < r0 + k; r++)
            for (int64_t e = off[r]; e < off[r + 1]; e++) all.push_back({times[e], r, e});
          std::sort(all.begin(), all.end());
          // 2. admission
          for (int64_t P : {0, 1, 2, 16})
            for (int64_t ms : durs) {
              std::vector<int64_t> admitted;
              for (const Fire& f : all) {
                int64_t busy = 0;
                for (size_t i = admitted.size(); busy < P && i-- > 0 && running(admitted[i], ms, f.t);) busy++;
                if (P == 0 || busy < P) {
                  admitted.push_back(f.t);
                  want[size_t(f.pos)] = 0;
                } else {
                  want[size_t(f.pos)] = kVerdictDropped;
                  dropped_all++;
                }
              }
              const int64_t d = inflight_seconds(ms, t1 - t0);
              const bool walk = !admit_never_drops(P, d, k);
              std::fill(got.begin() + off[r0], got.begin() + off[r0 + k], walk ? kVerdictDropped : 0);  // k_verdict_init
              if (walk) {
                admit_walks++;
                int64_t ring[kAdmitMaxParallels], wt[kAdmitWalkSlots];
                int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                const AdmitUnit u{r0, d, int32_t(k), int32_t(P)};
                admit_walk_unit(specs.data(), zv, plan.segs.data(), G, anc.data(), cnt.data(), dm.data(), t0, t1, u, ring, 1,
                                wc, [&](int64_t r, int64_t t) {
                                  if (r < r0 || r >= r0 + k) { bad++; return; }
                                  clear(r, t, kVerdictDropped);
                                });
              }
              compare(r0, k, "admission", (long long)P, (long long)ms, 0);
            }
          // 3. lock
          for (int kind : {JOB_ALONE, JOB_INTERVAL})
            for (int ai = 0; ai < int(sizeof avgs / sizeof avgs[0]); ai++) {
              const int64_t avg = avgs[ai];
              const int li = (horizons + ai + kind) % 3;
              const int64_t lock_ttl = ttls[li];
              const int hole = int(combo % 4);  // 0: all contend; 1, 2, 3: not the first, middle, last rule
              combo++;
              std::vector<uint8_t> cont(size_t(R), 1);
              if (hole) cont[size_t(r0 + (hole == 1 ? 0 : hole == 2 ? k / 2 : k - 1))] = 0;
              bool have_free = false, any = false;
              int64_t free_s = 0, free_ms = 0;  // the lease ends at free_s * 1000 + free_ms (no overflow at INT64_MAX ms)
              int64_t want_stuck = -1;
              for (int64_t r = r0; r < r0 + k; r++) any = any || cont[size_t(r)];
              for (const Fire& f : all) {
                want[size_t(f.pos)] = 0;
                if (!cont[size_t(f.rule)] || want_stuck >= 0) continue;
                if (have_free && (f.t - free_s < free_ms / 1000 || (f.t - free_s == free_ms / 1000 && free_ms % 1000 != 0))) {
                  want[size_t(f.pos)] = kVerdictSkipped;
                  skipped_all++;
                  continue;
                }
                const int64_t ttl = oracle_ttl(src[size_t(f.rule)], f.t, kind, ai, li);
                if (ttl == OR_NO_PROGRESS) { want_stuck = f.rule; continue; }
                if (ttl == 0) {
                  want[size_t(f.pos)] = kVerdictSkipped;
                  skipped_all++;
                  continue;
                }
                have_free = true;
                free_s = f.t + ttl;
                free_ms = kind == JOB_ALONE && avg > 0 ? avg : 0;
              }
              for (int64_t r = r0; r < r0 + k; r++)  // k_verdict_init: contending rules of a lock unit
                std::fill(got.begin() + off[r], got.begin() + off[r + 1], cont[size_t(r)] ? kVerdictSkipped : 0);
              int64_t got_stuck = -1;
              if (any) {
                lock_walks++;
                int64_t wt[kAdmitWalkSlots];
                int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                const LockUnit u{r0, avg, inflight_seconds(std::max<int64_t>(avg, 0), t1 - t0), int32_t(k), kind};
                got_stuck = lock_walk_unit(specs.data(), zv, plan.segs.data(), G, anc.data(), cnt.data(), dm.data(), t0, t1, u,
                                           lock_ttl, cont.data(), wc, [&](int64_t r, int64_t t) {
                                             if (r < r0 || r >= r0 + k || !cont[size_t(r)]) { bad++; return; }
                                             clear(r, t, kVerdictSkipped);
                                           });
              }
              if (got_stuck != want_stuck) {
                if (bad++ < 10)
                  printf("STUCK rule %lld vs %lld: %s unit [%s..] k=%lld t0=%lld w=%lld B=%d\n", (long long)got_stuck,
                         (long long)want_stuck, zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, sh.B);
                continue;
              }
              if (want_stuck >= 0) { stuck_walks++; continue; }  // the call fails: no bytes on either side
              compare(r0, k, "lock", kind, (long long)avg, (long long)lock_ttl);
            }
        }
    }
  printf("%s: %d of %d horizons skipped (non-terminating reference loop)\n", zone, skipped_h, horizons);
  if (4 * skipped_h > horizons) {
    printf("%s: more than a quarter of the horizons skipped\n", zone);
    bad++;
  }
  printf("%s: %d mismatches, %lld positions checked, %lld of them in walked runs; %lld bytes compared, %lld admission walks, "
         "%lld fires dropped, %lld lock walks, %lld fires skipped, %lld stuck walks\n",
         zone, bad, positions, walked_positions, bytes, admit_walks, dropped_all, lock_walks, skipped_all, stuck_walks);
  or_loc_free(ol);
  return bad ? 1 : 0;
}
