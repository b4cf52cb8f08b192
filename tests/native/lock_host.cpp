// Host-side check of the lock profile algorithm (cg_lock.h: lock_walk_unit over
// the run records of count_rule, with admit_fire_after's closed forms, walked
// runs and skips, two next_exact calls past the horizon per fire that finds
// the key gone, lock_ttl_of -- exactly what k_lock_units runs, over the zone
// table a lock profile stages; the start rows from profile_cell and the
// next_exact walk as k_profile_rules / k_profile_walk leave them) against the
// literal process of the definition run fire by fire over the oracle's Next
// loop with the oracle's or_lock_ttl at now = t: a unit's contending fires in
// (time, rule) order, one skipped iff t * 1000 < the lease's end in ms or its
// ttl is 0.
// Zones, specs, t0 choices and shapes are admit_host.cpp's; the rules of a
// horizon are grouped into units of 1, 2, 5 and 9, every unit is checked in
// both lock kinds with every avg_ms below, in both profile kinds; lock_ttl in
// {2, 300, 600} cycles over (horizon, kind, avg_ms) and a non-contending first,
// middle or last rule (or none) over the combinations.  With the zone argument Pacific/Apia
// the program instead checks that a fire whose Next never returns is reported.
// Test infrastructure; the GPU tests check the kernels themselves.
#include <algorithm>
#include <cstdlib>
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

struct Horizon {
  Plan plan;
  ZoneView zv;
  int G;
};

static void plan_of(const ZoneRules& zr, int64_t t0, int64_t t1, Horizon* h) {
  h->plan = build_plan(zr, t0, t1);
  h->plan.table = build_lock_table(zr, t0, t1);  // as run_set_count_scan stages it
  h->zv = ZoneView{h->plan.table.when.data(), h->plan.table.off.data(), int32_t(h->plan.table.when.size())};
  h->G = int(h->plan.segs.size());
}

// Pacific/Apia, 2011-12-15 00:00:17 UTC + 96 h: `0 0 9 * * Sat` fires on the
// 17th, its Next is the 24th, and the Next of that walks into the skipped
// 2011-12-30 and never returns -- the expansion itself ends (t1 is the 19th).
static int apia_stuck() {
  ZoneRules zr;
  or_loc* ol = nullptr;
  load_zone("Pacific/Apia", &zr, &ol);
  const char* names[] = {"0 0 12 * * *", "0 0 9 * * Sat", "@every 7200s"};
  std::vector<or_sched> scheds(3);
  char err[256];
  for (int i = 0; i < 3; i++)
    if (or_parse(OR_OPT_DEFAULT, names[i], strlen(names[i]), &scheds[i], err, sizeof err)) return 1;
  const int64_t t0 = 1323907217, w = 3600, t1 = t0 + 96 * w;
  Horizon h;
  plan_of(zr, t0, t1, &h);
  const int G = h.G;
  std::vector<DSpec> specs;
  std::vector<int64_t> anc(size_t(3) * G);
  std::vector<int32_t> cnt(size_t(3) * G);
  std::vector<uint32_t> dm(size_t(3) * G);
  int bad = 0;
  long long oracle_stuck = 0;
  for (int r = 0; r < 3; r++) {
    specs.push_back(pack(scheds[r]));
    if (or_expand(&scheds[r], t0, t1, ol, nullptr, 0) < 0) { printf("Apia: rule %d: the expansion is stuck\n", r); bad++; }
    if (!count_rule(specs[r], h.zv, h.plan.segs.data(), G, h.plan.dtab.data(), t0, t1, h.plan.flags, anc.data() + r * G,
                    cnt.data() + r * G, dm.data() + r * G)) { printf("Apia: count_rule: rule %d stuck\n", r); bad++; }
  }
  if (bad) return bad;
  std::vector<int64_t> buf(4096);
  for (int kind : {JOB_ALONE, JOB_INTERVAL})
    for (int usz : {1, 3}) {
      // units of one rule: only rule 1 is stuck; one unit of three: rule 1 too
      for (int r0 = 0; r0 < 3; r0 += usz) {
        int64_t want = -1;
        std::vector<std::pair<int64_t, int32_t>> fires;
        for (int r = r0; r < r0 + usz; r++) {
          const int64_t n = or_expand(&scheds[r], t0, t1, ol, buf.data(), 4096);
          for (int64_t i = 0; i < n; i++) fires.push_back({buf[i], r});
        }
        std::sort(fires.begin(), fires.end());
        int64_t free_ms = INT64_MIN;
        for (const auto& f : fires) {
          if (f.first * 1000 < free_ms) continue;
          const int64_t ttl = or_lock_ttl(&scheds[f.second], f.first, 0, ol, kind, 1000, 300);
          if (ttl == OR_NO_PROGRESS) { want = f.second; oracle_stuck++; break; }
          if (ttl == 0) continue;
          free_ms = f.first * 1000 + ttl * 1000 + (kind == JOB_ALONE ? 1000 : 0);
        }
        int64_t wt[kAdmitWalkSlots];
        int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
        const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
        const LockUnit u{r0, 1000, 1, usz, kind};
        const int64_t got = lock_walk_unit(specs.data(), h.zv, h.plan.segs.data(), G, anc.data(), cnt.data(), dm.data(), t0,
                                           t1, u, 300, nullptr, wc, [](int64_t, int64_t) {});
        if (got != want) {
          printf("Apia: unit [%d, %d) kind %d: stuck rule %lld vs the oracle's %lld\n", r0, r0 + usz, kind, (long long)got,
                 (long long)want);
          bad++;
        }
      }
    }
  printf("Pacific/Apia: %d mismatches, %lld walks the oracle's lockTtl never returns from\n", bad, oracle_stuck);
  or_loc_free(ol);
  return bad || oracle_stuck == 0 ? 1 : 0;
}

int main(int argc, char** argv) {
  const char* zone = argc > 1 ? argv[1] : "UTC";
  if (!strcmp(zone, "Pacific/Apia")) return apia_stuck();
  const int nspec = argc > 2 ? atoi(argv[2]) : 60;
  // as profile_host.cpp: a rule is checked on a horizon only where it fires at
  // most kRuleCap times there, a horizon's spec list is cut at `budget` fires.
  // Every fire is visited in 64 combinations here, so one rule gets at most
  // the budget: an every-second rule is left to the horizons of some hours.
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
  long long total = 0, cells = 0, walked_fires = 0, unit_walks = 0, granted_all = 0, skipped_all = 0, stuck_walks = 0;
  LockWalkStats stats;
  unsigned combo = 0;
  for (int64_t t0 : t0s)
    for (const Shape& sh : shapes) {
      const int64_t w = sh.w, t1 = t0 + sh.B * w;
      const int32_t B = sh.B;
      horizons++;
      Horizon h;
      plan_of(zr, t0, t1, &h);
      const int G = h.G;
      const ZoneView& zv = h.zv;
      const Plan& plan = h.plan;
      {
        // the longer table must leave the horizon's own lookups as they were
        const Plan own = build_plan(zr, t0, t1);
        const ZoneView ov{own.table.when.data(), own.table.off.data(), int32_t(own.table.when.size())};
        for (int64_t x = t0 - 64 * 86400; x <= t1 + (6 * 366 + 64) * 86400; x += 1 + (t1 + 6 * 366 * 86400 - t0) / 5000)
          if (zone_offset(ov, x) != zone_offset(zv, x) && bad++ < 10)
            printf("TABLE mismatch %s at %lld\n", zone, (long long)x);
      }
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
      // the used rules, compacted: specs, run records at stride G, start rows
      std::vector<DSpec> specs;
      std::vector<size_t> src;
      std::vector<int64_t> anc;
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
          if (bad++ < 10) printf("STUCK mismatch %s [%s] t0=%lld w=%lld B=%d\n", zone, names[r].c_str(), (long long)t0, (long long)w, B);
          anc.resize(j0);
          cnt.resize(j0);
          dm.resize(j0);
          continue;
        }
        for (int s = 0; s < G; s++)
          if (cnt[j0 + s] && !run_has_closed_form(d, plan.segs[s], dm[j0 + s])) walked_fires += cnt[j0 + s];
        specs.push_back(d);
        src.push_back(r);
      }
      const int64_t R = int64_t(specs.size());
      std::vector<int32_t> starts(size_t(R) * B, 0);
      for (int64_t r = 0; r < R; r++) {
        const CFRule c = cf_rule(specs[r]);
        const size_t j0 = size_t(r) * G;
        int32_t* row = starts.data() + r * B;
        for (int32_t b = 0; b < B; b++)
          row[b] = profile_cell(specs[r], c, plan.segs.data(), G, anc.data() + j0, cnt.data() + j0, dm.data() + j0, t1,
                                t0 + b * w, t0 + (b + 1) * w);
        for (int s = 0; s < G; s++) {  // k_profile_walk
          if (cnt[j0 + s] == 0 || run_has_closed_form(specs[r], plan.segs[s], dm[j0 + s])) continue;
          int64_t t = anc[j0 + s];
          for (int k = 0; k < cnt[j0 + s]; k++) {
            t = next_exact(specs[r], zv, t, t1);
            row[(t - t0 - 1) / w]++;
          }
        }
      }
      // or_lock_ttl is two literal Next loops, microseconds each in a zone, and the same (rule, fire, kind,
      // avg, lock_ttl) is asked again by the other unit sizes: its answers are kept for the horizon
      std::unordered_map<uint64_t, int64_t> memo;
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
          for (int kind : {JOB_ALONE, JOB_INTERVAL})
            for (int ai = 0; ai < int(sizeof avgs / sizeof avgs[0]); ai++) {
              const int64_t avg = avgs[ai];
              // lock_ttl cycles with the horizon, so a fire's ttl is asked once for the four unit sizes
              const int li = (horizons + ai + kind) % 3;
              const int64_t lock_ttl = ttls[li];
              const int hole = int(combo % 4);  // 0: all contend; 1, 2, 3: not the first, middle, last rule
              combo++;
              std::vector<uint8_t> cont(size_t(R), 1);
              if (hole) cont[size_t(r0 + (hole == 1 ? 0 : hole == 2 ? k / 2 : k - 1))] = 0;
              // the literal process over the oracle
              std::vector<std::pair<int64_t, int32_t>> fires;
              for (int64_t r = r0; r < r0 + k; r++)
                if (cont[size_t(r)])
                  for (int64_t t : exp[src[r]]) fires.push_back({t, int32_t(r - r0)});
              std::sort(fires.begin(), fires.end());
              std::vector<int32_t> want_g(starts.begin() + r0 * B, starts.begin() + (r0 + k) * B);
              std::vector<int32_t> want_s(size_t(k) * B, 0);
              for (int64_t r = r0; r < r0 + k; r++)
                if (cont[size_t(r)]) std::fill(want_g.begin() + (r - r0) * B, want_g.begin() + (r - r0 + 1) * B, 0);
              bool have_free = false;
              int64_t free_s = 0, free_ms = 0;  // the lease ends at free_s * 1000 + free_ms (no overflow at INT64_MAX ms)
              int64_t want_stuck = -1;
              for (const auto& f : fires) {
                const int64_t cell = int64_t(f.second) * B + (f.first - t0 - 1) / w;
                // t * 1000 < end  <=>  t < free_s + free_ms / 1000, or equal seconds and a remainder
                if (have_free && (f.first - free_s < free_ms / 1000 || (f.first - free_s == free_ms / 1000 && free_ms % 1000 != 0))) {
                  want_s[cell]++;
                  skipped_all++;
                  continue;
                }
                const int64_t ttl = oracle_ttl(src[r0 + f.second], f.first, kind, ai, li);
                if (ttl == OR_NO_PROGRESS) { want_stuck = r0 + f.second; break; }
                if (ttl == 0) {
                  want_s[cell]++;
                  skipped_all++;
                  continue;
                }
                want_g[cell]++;
                granted_all++;
                have_free = true;
                free_s = f.first + ttl;
                free_ms = kind == JOB_ALONE && avg > 0 ? avg : 0;
              }
              // the engine's way: both kinds from the start rows
              std::vector<int32_t> got_g(starts.begin() + r0 * B, starts.begin() + (r0 + k) * B);
              std::vector<int32_t> got_s(size_t(k) * B, 0);
              int64_t got_stuck = -1;
              if (!fires.empty() || std::any_of(cont.begin() + r0, cont.begin() + r0 + k, [](uint8_t c) { return c; })) {
                unit_walks++;
                for (int64_t r = r0; r < r0 + k; r++)
                  if (cont[size_t(r)]) {  // k_admit_prepare: GRANTED zeroes the flagged rows, SKIPPED keeps only them
                    std::copy(got_g.begin() + (r - r0) * B, got_g.begin() + (r - r0 + 1) * B, got_s.begin() + (r - r0) * B);
                    std::fill(got_g.begin() + (r - r0) * B, got_g.begin() + (r - r0 + 1) * B, 0);
                  }
                int64_t wt[kAdmitWalkSlots];
                int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                const LockUnit u{r0, avg, inflight_seconds(std::max<int64_t>(avg, 0), int64_t(B) * w), int32_t(k), kind};
                got_stuck = lock_walk_unit(specs.data(), zv, plan.segs.data(), G, anc.data(), cnt.data(), dm.data(), t0, t1, u,
                                           lock_ttl, cont.data(), wc,
                                           [&](int64_t r, int64_t t) {
                                             const int64_t b = (t - t0 - 1) / w;
                                             if (t <= t0 || b >= B || r < r0 || r >= r0 + k || !cont[size_t(r)]) { bad++; return; }
                                             got_g[(r - r0) * B + b] += 1;
                                             got_s[(r - r0) * B + b] -= 1;
                                           },
                                           &stats);
              }
              if (got_stuck != want_stuck) {
                if (bad++ < 10)
                  printf("STUCK rule %lld vs %lld: %s unit [%s..] k=%lld t0=%lld w=%lld B=%d\n", (long long)got_stuck,
                         (long long)want_stuck, zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, B);
                continue;
              }
              if (want_stuck >= 0) { stuck_walks++; continue; }  // the rows are unfinished on both sides
              cells += 2 * k * B;
              if ((got_g != want_g || got_s != want_s) && bad++ < 10) {
                size_t i = 0;
                while (got_g[i] == want_g[i] && got_s[i] == want_s[i]) i++;
                printf("MISMATCH %s unit [%s..] k=%lld t0=%lld w=%lld B=%d kind=%d avg=%lld ms lock_ttl=%lld hole=%d rule +%zu "
                       "bucket %zu: granted %d vs %d, skipped %d vs %d (G=%d)\n",
                       zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, B, kind, (long long)avg,
                       (long long)lock_ttl, hole, i / B, i % B, got_g[i], want_g[i], got_s[i], want_s[i], G);
              }
            }
        }
    }
  printf("%s: %d of %d horizons skipped (non-terminating reference loop)\n", zone, skipped_h, horizons);
  if (4 * skipped_h > horizons) {
    printf("%s: more than a quarter of the horizons skipped\n", zone);
    bad++;
  }
  printf("%s: %d mismatches, %lld cells, %lld events checked, %lld of them walked; %lld unit walks, %lld fires granted, "
         "%lld fires skipped, %lld skip-ahead jumps, %lld ttl evaluations, %lld with a Next past t1, %lld with ttl 0, "
         "%lld stuck walks\n",
         zone, bad, cells, total, walked_fires, unit_walks, granted_all, skipped_all, stats.jumps, stats.ttl_evals,
         stats.ttl_past, stats.ttl_zero, stuck_walks);
  or_loc_free(ol);
  return bad ? 1 : 0;
}
