/*
 * abi_lock_c.c -- the lock profile entry points of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on a ten-rule set, in the call
 * order of the cgo stub's LockProfile / LockProfilePerNode:
 * cg_lock_profile_device, cg_profile_kind, cg_profile_copy_rules,
 * cg_profile_copy_totals, cg_lock_profile_per_node_device,
 * cg_profile_copy_nodes.
 * Test infrastructure: tests/test_abi_lock_c.py compiles it with
 * `gcc -std=c11 -pedantic -Werror` and compares what it prints with the model.
 *
 *   abi_lock_c <zoneinfo dir>      "K key values..." lines
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

static const char* kSpecs[] = {"0 */5 * * * *",  "0 30 9 * * 1-5", "*/10 * * * * *",    "*/15 * * * * *", "@every 60s",
                               "0 0 0 30 Feb ?", "0 30 2 * * *",   "7,30,45 * * * * *", "@every 7s",      "* * * * * *"};
#define NSPEC ((int)(sizeof kSpecs / sizeof kSpecs[0]))
#define WIDTH 1800
#define NB 24
#define LOCK_TTL 300
/* units {0,1} {2,3} {4} {5,6} {7,8} {9}: kind, AvgTime, unit and contends per rule */
static const int32_t kKind[NSPEC] = {CG_JOB_INTERVAL, CG_JOB_INTERVAL, CG_JOB_ALONE,    CG_JOB_ALONE,    CG_JOB_ALONE,
                                     CG_JOB_COMMON,   CG_JOB_COMMON,   CG_JOB_INTERVAL, CG_JOB_INTERVAL, CG_JOB_ALONE};
static const int64_t kAvg[NSPEC] = {400000, 400000, 25000, 25000, 2500, 0, 0, -1500, -1500, INT64_MAX};
static const int32_t kUnit[NSPEC] = {0, 0, 3, 3, 4, 7, 7, 8, 8, 9};
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (cg_abi_version() != CG_ABI_VERSION || CG_ABI_VERSION != 3) return 4;
  if (CG_PROFILE_LOCK_GRANTED != 4 || CG_PROFILE_LOCK_SKIPPED != 5) return 5;
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

  /* one job per unit; the rules of a job differ in membership */
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
    const char* gids[] = {i % 2 ? "g1" : "g2"};
    const char* nids[] = {"n5"};
    const char* ex[] = {"n3"};
    CHECK(cg_jobset_add_rule(js, rid, gids, (size_t)(i != 3), nids, (size_t)(i % 3 == 0 && i != 3), ex, 0));
  }
  cg_rules_in rin;
  CHECK(cg_jobset_rules(js, &rin));
  printf("J rules %d nodes %d\n", rin.n_rules, rin.n_nodes);

  /* the argument checks need no device: a null context is refused like the rest */
  if (cg_lock_profile_device(NULL, NULL, NULL, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL,
                             CG_PROFILE_LOCK_SKIPPED) != CG_EINVAL)
    return 30;
  if (cg_lock_profile_per_node_device(NULL, NULL, NULL, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL,
                                      CG_PROFILE_LOCK_GRANTED, NULL, 0) != CG_EINVAL)
    return 31;

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

  /* refusals come before any device work */
  int kind = -1;
  int64_t bad[NSPEC];
  int32_t kbad[NSPEC], ubad[NSPEC];
  const int S = CG_PROFILE_LOCK_SKIPPED, G = CG_PROFILE_LOCK_GRANTED;
  if (cg_lock_profile_device(ctx, sp, ny, 0, 0, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 7;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, 4097, kKind, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 8;
  if (cg_lock_profile_device(ctx, sp, ny, 0, CG_MAX_HORIZON, 2, kKind, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_ERANGE)
    return 9;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, NULL, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 10;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, NULL, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 11;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, CG_PROFILE_DROPPED) !=
      CG_EINVAL)
    return 12;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, 6) != CG_EINVAL) return 13;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, 1, S) != CG_EINVAL) return 14;
  memcpy(kbad, kKind, sizeof kbad);
  kbad[6] = 3;
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kbad, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 15;
  if (!strstr(cg_last_error(), "rule 6:")) return 16;
  memcpy(ubad, kUnit, sizeof ubad);
  ubad[4] = 2; /* 0 0 3 3 2: decreases */
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, ubad, kContends, LOCK_TTL, S) != CG_EINVAL) return 17;
  if (!strstr(cg_last_error(), "rule 4:")) return 18;
  memcpy(bad, kAvg, sizeof bad);
  bad[8] = 15; /* differs from rule 7 of the same unit */
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kKind, bad, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 19;
  if (!strstr(cg_last_error(), "rule 8:")) return 20;
  memcpy(kbad, kKind, sizeof kbad);
  kbad[1] = CG_JOB_ALONE; /* differs from rule 0 of the same unit */
  if (cg_lock_profile_device(ctx, sp, ny, 0, WIDTH, NB, kbad, kAvg, kUnit, kContends, LOCK_TTL, S) != CG_EINVAL) return 21;
  if (!strstr(cg_last_error(), "rule 1:")) return 22;
  if (cg_lock_profile_per_node_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, G, NULL, 0) !=
      CG_EINVAL)
    return 24;
  if (cg_lock_profile_per_node_device(ctx, sp, ny, 0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, G, rules, 3) !=
      CG_EINVAL)
    return 25;
  if (cg_profile_kind(ctx, &kind) != CG_EINVAL) return 26; /* nothing readable yet */

  /* six hours before the 2026-03-08 spring-forward, at a non-aligned second */
  const int64_t t0 = 1772953200LL - 6 * 3600 + 17;
  static int32_t rows[NSPEC * NB];
  static int64_t totals[NB], nodes[16 * NB];
  for (int pass = 0; pass < 2; pass++) {
    CHECK(cg_lock_profile_device(ctx, sp, ny, t0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, pass ? G : S));
    CHECK(cg_profile_kind(ctx, &kind));
    printf("K %d\n", kind);
    CHECK(cg_profile_copy_rules(ctx, 0, NSPEC, rows));
    CHECK(cg_profile_copy_totals(ctx, totals));
    for (int r = 0; r < NSPEC; r++) {
      printf(pass ? "G" : "S");
      for (int b = 0; b < NB; b++) printf(" %d", rows[r * NB + b]);
      printf("\n");
    }
    printf(pass ? "T" : "U");
    for (int b = 0; b < NB; b++) printf(" %lld", (long long)totals[b]);
    printf("\n");
  }
  float ms[22];
  if (cg_last_kernel_times(ctx, ms, 22) != 22 || !(ms[21] > 0.f) || ms[20] != 0.f) return 27;

  if (rin.n_nodes > 16) return 28;
  CHECK(cg_lock_profile_per_node_device(ctx, sp, ny, t0, WIDTH, NB, kKind, kAvg, kUnit, kContends, LOCK_TTL, S, rules,
                                        CG_EXCLUDE_NONE));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  CHECK(cg_profile_copy_nodes(ctx, 0, rin.n_nodes, nodes));
  for (int n = 0; n < rin.n_nodes; n++) {
    printf("M %s", cg_jobset_node_id(js, n));
    for (int b = 0; b < NB; b++) printf(" %lld", (long long)nodes[n * NB + b]);
    printf("\n");
  }
  /* a start profile replaces it */
  CHECK(cg_profile_device(ctx, sp, ny, t0, WIDTH, NB));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  printf("OK\n");
  cg_rules_free(rules);
  cg_specs_free(sp);
  cg_destroy(ctx);
  cg_jobset_free(js);
  cg_zone_free(ny);
  return 0;
}
