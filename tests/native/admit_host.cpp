// Host-side check of the admission profile algorithm (cg_admit.h:
// admit_walk_unit over the run records of count_rule, with admit_fire_after's
// closed forms, walked runs and skips -- exactly what k_admit_units runs; the
// start rows from profile_cell and the next_exact walk as k_profile_rules /
// k_profile_walk leave them) against the literal process of the definition run
// fire by fire over the oracle's Next loop: a unit's fires in (time, rule)
// order, one admitted iff fewer than P admitted fires a have
// a * 1000 + dur_ms > t * 1000.
// Zones, specs, t0 choices and shapes are profile_host.cpp's; the rules of a
// horizon are grouped into units of 1, 2, 5 and 9 and every unit is checked with
// P in {0, 1, 2, 16} and inflight_host.cpp's durations, in both kinds.
// Test infrastructure; the GPU tests check the kernels themselves.
#include <algorithm>
#include <cstdlib>
#include <random>

#include "../../cronsun_amd/csrc/cg_admit.h"
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

// is a command started at a with a run time of ms still running at t >= a?
static bool running(int64_t a, int64_t ms, int64_t t) {
  return ms / 1000 > t - a || (ms / 1000 == t - a && ms % 1000 != 0);  // a * 1000 + ms > t * 1000
}

int main(int argc, char** argv) {
  const char* zone = argc > 1 ? argv[1] : "UTC";
  const int nspec = argc > 2 ? atoi(argv[2]) : 60;
  // as profile_host.cpp: a rule is checked on a horizon only where it fires at
  // most kRuleCap times there, a horizon's spec list is cut at `budget` fires
  const long long budget = argc > 4 ? atoll(argv[4]) : 300000;
  const int64_t kRuleCap = 200000;
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
  int bad = 0, skipped = 0, horizons = 0;
  long long total = 0, cells = 0, walked_fires = 0, units_walked = 0, units_plain = 0, dropped_all = 0;
  for (int64_t t0 : t0s)
    for (const Shape& sh : shapes) {
      const int64_t w = sh.w, t1 = t0 + sh.B * w;
      const int32_t B = sh.B;
      const int64_t durs[] = {0, 1, 999, 1000, 1001, w * 1000 - 1, w * 1000, w * 1000 + 1, 3500 * w,
                              45LL * 86400 * 1000, INT64_MAX};
      horizons++;
      Plan plan = build_plan(zr, t0, t1);
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
      if (stuck) { skipped++; continue; }
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
      for (int usz : {1, 2, 5, kAdmitWalkSlots + 1})  // the last: two rules share a remembered position
        for (int64_t r0 = 0; r0 < R; r0 += usz) {
          const int64_t k = std::min<int64_t>(usz, R - r0);
          // the unit's fires in (time, rule) order, from the oracle
          std::vector<std::pair<int64_t, int32_t>> fires;
          for (int64_t r = r0; r < r0 + k; r++)
            for (int64_t t : exp[src[r]]) fires.push_back({t, int32_t(r - r0)});
          std::sort(fires.begin(), fires.end());
          for (int64_t P : {0, 1, 2, 16})
            for (int64_t ms : durs) {
              // the literal process
              std::vector<int32_t> want_adm(size_t(k) * B, 0), want_drop(size_t(k) * B, 0);
              std::vector<int64_t> admitted;
              for (const auto& f : fires) {
                int64_t busy = 0;
                // (admitted is ascending: the running ones are its tail; P of them settle it)
                for (size_t i = admitted.size(); busy < P && i-- > 0 && running(admitted[i], ms, f.first);) busy++;
                const int64_t cell = int64_t(f.second) * B + (f.first - t0 - 1) / w;
                if (P == 0 || busy < P) {
                  admitted.push_back(f.first);
                  want_adm[cell]++;
                } else {
                  want_drop[cell]++;
                  dropped_all++;
                }
              }
              // the engine's way: both kinds from the start rows
              const int64_t d = inflight_seconds(ms, int64_t(B) * w);
              std::vector<int32_t> got_adm(starts.begin() + r0 * B, starts.begin() + (r0 + k) * B);
              std::vector<int32_t> got_drop(size_t(k) * B, 0);
              if (!admit_never_drops(P, d, k)) {
                units_walked++;
                got_drop = got_adm;  // DROPPED: start - admitted
                std::fill(got_adm.begin(), got_adm.end(), 0);
                int64_t ring[kAdmitMaxParallels], wt[kAdmitWalkSlots];
                int32_t wrel[kAdmitWalkSlots], ws[kAdmitWalkSlots], wq[kAdmitWalkSlots];
                const AdmitWalkCache wc{wt, wrel, ws, wq, 1};
                const AdmitUnit u{r0, d, int32_t(k), int32_t(P)};
                admit_walk_unit(specs.data(), zv, plan.segs.data(), G, anc.data(), cnt.data(), dm.data(), t0, t1, u,
                                ring, 1, wc, [&](int64_t r, int64_t t) {
                                  const int64_t b = (t - t0 - 1) / w;
                                  if (t <= t0 || b >= B || r < r0 || r >= r0 + k) { bad++; return; }
                                  got_adm[(r - r0) * B + b] += 1;
                                  got_drop[(r - r0) * B + b] -= 1;
                                });
              } else {
                units_plain++;
              }
              cells += 2 * k * B;
              if ((got_adm != want_adm || got_drop != want_drop) && bad++ < 10) {
                size_t i = 0;
                while (got_adm[i] == want_adm[i] && got_drop[i] == want_drop[i]) i++;
                printf("MISMATCH %s unit [%s..] k=%lld t0=%lld w=%lld B=%d P=%lld dur=%lld ms rule +%zu bucket %zu: "
                       "admitted %d vs %d, dropped %d vs %d (G=%d)\n",
                       zone, names[src[r0]].c_str(), (long long)k, (long long)t0, (long long)w, B, (long long)P,
                       (long long)ms, i / B, i % B, got_adm[i], want_adm[i], got_drop[i], want_drop[i], G);
              }
            }
        }
    }
  printf("%s: %d of %d horizons skipped (non-terminating reference loop)\n", zone, skipped, horizons);
  if (4 * skipped > horizons) {
    printf("%s: more than a quarter of the horizons skipped\n", zone);
    bad++;
  }
  printf("%s: %d mismatches, %lld cells, %lld events checked, %lld of them walked; %lld unit walks, %lld units that never "
         "drop, %lld fires dropped\n",
         zone, bad, cells, total, walked_fires, units_walked, units_plain, dropped_all);
  or_loc_free(ol);
  return bad ? 1 : 0;
}
