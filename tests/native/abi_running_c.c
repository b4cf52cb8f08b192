/*
 * abi_running_c.c -- the running profile kinds of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on abi_admit_c.c's ten-rule
 * set: cg_admit_device and cg_admit_per_node_device with CG_PROFILE_RUNNING,
 * cg_lock_profile_device with CG_PROFILE_LOCK_RUNNING, then cg_profile_kind,
 * the copy accessors, cg_profile_node_peaks and cg_last_kernel_times [22].
 * Test infrastructure: tests/test_abi_running_c.py compiles it with
 * `gcc -std=c11 -pedantic -Werror` and compares what it prints with the model.
 *
 *   abi_running_c <zoneinfo dir>      "K key values..." lines
 *
 * Without a gfx950 device cg_init fails with CG_ENODEV and the program
 * prints "NODEV".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cronsun_gpu.h"

#define CHECK(x)                                                                  \
  do {                                                                            \
    int rc_ = (x);                                                                \
    if (rc_ != CG_OK) {                                                           \
      fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #x, rc_,      \
              cg_last_error());                                                   \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static const char* kSpecs[] = {"0 */5 * * * *",  "0 30 9 * * 1-5", "*/10 * * * * *",    "*/15 * * * * *", "@every 90s",
                               "0 0 0 30 Feb ?", "0 30 2 * * *",   "7,30,45 * * * * *", "@every 7s",      "* * * * * *"};
#define NSPEC ((int)(sizeof kSpecs / sizeof kSpecs[0]))
#define WIDTH 1800
#define NB 24
#define LOCK_TTL 300
/* units {0,1} {2,3} {4} {5,6} {7,8} {9}: ms (the lock flavour's AvgTime), limit, unit and Job.Kind per rule */
static const int64_t kDur[NSPEC] = {400000, 400000, 25000, 25000, 1800000, 0, 0, 20000, 20000, INT64_MAX};
static const int64_t kPar[NSPEC] = {1, 1, 2, 2, 1, 1, 1, 16, 16, 2};
static const int32_t kUnit[NSPEC] = {0, 0, 3, 3, 4, 7, 7, 8, 8, 9};
static const int32_t kKind[NSPEC] = {CG_JOB_ALONE,    CG_JOB_ALONE,    CG_JOB_INTERVAL, CG_JOB_INTERVAL, CG_JOB_COMMON,
                                     CG_JOB_INTERVAL, CG_JOB_INTERVAL, CG_JOB_ALONE,    CG_JOB_ALONE,    CG_JOB_ALONE};
static const uint8_t kContends[NSPEC] = {1, 1, 1, 0, 1, 1, 1, 1, 1, 1};

static unsigned char* read_file(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* b = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);
  *len = fread(b, 1, (size_t)(n > 0 ? n : 0), f);
  fclose(f);
  return b;
}

static void print_rows(const char* key, const int32_t* rows, const char* tkey, const int64_t* totals) {
  for (int r = 0; r < NSPEC; r++) {
    printf("%s", key);
    for (int b = 0; b < NB; b++) printf(" %d", rows[r * NB + b]);
    printf("\n");
  }
  printf("%s", tkey);
  for (int b = 0; b < NB; b++) printf(" %lld", (long long)totals[b]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (cg_abi_version() != CG_ABI_VERSION) return 4;
  if (CG_PROFILE_RUNNING != 7 || CG_PROFILE_LOCK_RUNNING != 8) return 5;
  cg_schedule sched[NSPEC];
  char err[256];
  for (int i = 0; i < NSPEC; i++)
    CHECK(cg_parse(CG_PARSE_DEFAULT, kSpecs[i], strlen(kSpecs[i]), &sched[i], err, sizeof err));
  char path[1024];
  snprintf(path, sizeof path, "%s/America/New_York", argv[1]);
  size_t zlen = 0;
  unsigned char* tzif = read_file(path, &zlen);
  if (!tzif) return 6;
  cg_zone* ny;
  CHECK(cg_zone_from_tzif(tzif, zlen, &ny));
  free(tzif);

  /* one job per unit, so the rules of a unit run on the same nodes */
  cg_jobset* js;
  CHECK(cg_jobset_new(&js));
  const char* g1[] = {"n1", "n2", "n3"};
  const char* g2[] = {"n3", "n4"};
  CHECK(cg_jobset_add_group(js, "g1", g1, 3));
  CHECK(cg_jobset_add_group(js, "g2", g2, 2));
  for (int i = 0, job = 0; i < NSPEC; i++) {
    if (i == 0 || kUnit[i] != kUnit[i - 1]) {
      char id[16];
      snprintf(id, sizeof id, "job%d", job++);
      CHECK(cg_jobset_add_job(js, id, 0));
    }
    char rid[16];
    snprintf(rid, sizeof rid, "r%d", i);
    const char* gids[] = {kUnit[i] % 2 ? "g1" : "g2"};
    const char* nids[] = {"n5"};
    const char* ex[] = {"n3"};
    CHECK(cg_jobset_add_rule(js, rid, gids, 1, nids, (size_t)(kUnit[i] % 3 == 0), ex, 0));
  }
  cg_rules_in rin;
  CHECK(cg_jobset_rules(js, &rin));
  printf("J rules %d nodes %d\n", rin.n_rules, rin.n_nodes);

  cg_ctx* ctx = NULL;
  int rc = cg_init(0, &ctx);
  if (rc == CG_ENODEV) {
    printf("NODEV %s\n", cg_last_error());
    cg_jobset_free(js);
    cg_zone_free(ny);
    return 0;
  }
  CHECK(rc);
  cg_specs* sp;
  CHECK(cg_specs_upload_schedules(ctx, sched, NSPEC, &sp));
  cg_rules* rules;
  CHECK(cg_rules_upload(ctx, &rin, &rules));

  /* each entry point takes its own RUNNING kind only; 6 is not assigned; the
   * checks of the other kinds apply */
  const int RUN = CG_PROFILE_RUNNING, LRUN = CG_PROFILE_LOCK_RUNNING;
  int kind = -1;
  int64_t bad[NSPEC];
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, LRUN) != CG_EINVAL) return 7;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, 6) != CG_EINVAL) return 8;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kDur, kUnit, kContends, LOCK_TTL, RUN) != CG_EINVAL)
    return 9;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kDur, kUnit, kContends, LOCK_TTL, 6) != CG_EINVAL)
    return 10;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, 4097, kDur, kPar, kUnit, RUN) != CG_EINVAL) return 11;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, NULL, kPar, kUnit, RUN) != CG_EINVAL) return 12;
  memcpy(bad, kDur, sizeof bad);
  bad[3] = -1;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, bad, kPar, kUnit, RUN) != CG_EINVAL) return 13;
  if (!strstr(cg_last_error(), "rule 3:")) return 14;
  memcpy(bad, kPar, sizeof bad);
  bad[9] = 17; /* runs for ever, so 17 can drop */
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, bad, kUnit, RUN) != CG_ERANGE) return 15;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kDur, kUnit, kContends, 1, LRUN) != CG_EINVAL)
    return 16;
  if (cg_admit_per_node_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, RUN, NULL, 0) != CG_EINVAL) return 17;
  if (cg_profile_kind(ctx, &kind) != CG_EINVAL) return 18; /* nothing readable yet */

  /* six hours before the 2026-03-08 spring-forward, at a non-aligned second */
  const int64_t t0 = 1772953200LL - 6 * 3600 + 17;
  static int32_t rows[NSPEC * NB];
  static int64_t totals[NB], nodes[16 * NB], peak[16];
  static int32_t bucket[16];
  float ms[23];

  CHECK(cg_admit_device(ctx, sp, ny, t0, WIDTH, NB, kDur, kPar, kUnit, RUN));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  CHECK(cg_profile_copy_rules(ctx, 0, NSPEC, rows));
  CHECK(cg_profile_copy_totals(ctx, totals));
  print_rows("R", rows, "T", totals);
  if (cg_last_kernel_times(ctx, ms, 23) != 23 || !(ms[22] > 0.f) || !(ms[20] > 0.f) || ms[21] != 0.f) return 19;
  if (cg_profile_node_peaks(ctx, 0, 1, peak, bucket) != CG_EINVAL) return 20; /* no node matrix yet */

  CHECK(cg_lock_profile_device(ctx, sp, ny, t0, WIDTH, NB, kKind, kDur, kUnit, kContends, LOCK_TTL, LRUN));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  CHECK(cg_profile_copy_rules(ctx, 0, NSPEC, rows));
  CHECK(cg_profile_copy_totals(ctx, totals));
  print_rows("L", rows, "U", totals);
  if (cg_last_kernel_times(ctx, ms, 23) != 23 || !(ms[22] > 0.f) || !(ms[21] > 0.f) || ms[20] != 0.f) return 21;

  if (rin.n_nodes > 16) return 22;
  CHECK(cg_admit_per_node_device(ctx, sp, ny, t0, WIDTH, NB, kDur, kPar, kUnit, RUN, rules, CG_EXCLUDE_NONE));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  CHECK(cg_profile_copy_nodes(ctx, 0, rin.n_nodes, nodes));
  CHECK(cg_profile_node_peaks(ctx, 0, rin.n_nodes, peak, bucket));
  for (int n = 0; n < rin.n_nodes; n++) {
    printf("M %s", cg_jobset_node_id(js, n));
    for (int b = 0; b < NB; b++) printf(" %lld", (long long)nodes[n * NB + b]);
    printf("\n");
    printf("P %s %lld %d\n", cg_jobset_node_id(js, n), (long long)peak[n], bucket[n]);
  }
  /* an admitted profile replaces it, and its slot [22] reads 0 */
  CHECK(cg_admit_device(ctx, sp, ny, t0, WIDTH, NB, kDur, kPar, kUnit, CG_PROFILE_ADMITTED));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  if (cg_last_kernel_times(ctx, ms, 23) != 23 || ms[22] != 0.f) return 23;
  printf("OK\n");
  cg_rules_free(rules);
  cg_specs_free(sp);
  cg_destroy(ctx);
  cg_jobset_free(js);
  cg_zone_free(ny);
  return 0;
}
