/*
 * abi_admit_c.c -- the admission profile entry points of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on a ten-rule set, in the call
 * order of the cgo stub's Admit / AdmitPerNode / NodePeaks: cg_admit_device,
 * cg_profile_kind, cg_profile_copy_rules, cg_profile_copy_totals,
 * cg_admit_per_node_device, cg_profile_copy_nodes, cg_profile_node_peaks.
 * Test infrastructure: tests/test_abi_admit_c.py compiles it with
 * `gcc -std=c11 -pedantic -Werror` and compares what it prints with the model.
 *
 *   abi_admit_c <zoneinfo dir>      "K key values..." lines
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
/* units {0,1} {2,3} {4} {5,6} {7,8} {9}: ms, limit and unit per rule */
static const int64_t kDur[NSPEC] = {400000, 400000, 25000, 25000, 180001, 0, 0, 20000, 20000, INT64_MAX};
static const int64_t kPar[NSPEC] = {1, 1, 2, 2, 1, 1, 1, 16, 16, 2};
static const int32_t kUnit[NSPEC] = {0, 0, 3, 3, 4, 7, 7, 8, 8, 9};

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
  if (cg_abi_version() != CG_ABI_VERSION) return 4;
  if (CG_PROFILE_ADMITTED != 2 || CG_PROFILE_DROPPED != 3 || CG_ADMIT_MAX_PARALLELS != 16) return 5;
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

  /* refusals come before any device work */
  int kind = -1;
  int64_t bad[NSPEC];
  int32_t ubad[NSPEC];
  const int D = CG_PROFILE_DROPPED, A = CG_PROFILE_ADMITTED;
  if (cg_admit_device(ctx, sp, ny, 0, 0, NB, kDur, kPar, kUnit, D) != CG_EINVAL) return 7;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, 4097, kDur, kPar, kUnit, D) != CG_EINVAL) return 8;
  if (cg_admit_device(ctx, sp, ny, 0, CG_MAX_HORIZON, 2, kDur, kPar, kUnit, D) != CG_ERANGE) return 9;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, NULL, kPar, kUnit, D) != CG_EINVAL) return 10;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, NULL, kUnit, D) != CG_EINVAL) return 11;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, CG_PROFILE_INFLIGHT) != CG_EINVAL) return 12;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, 4) != CG_EINVAL) return 13;
  memcpy(bad, kDur, sizeof bad);
  bad[3] = -1;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, bad, kPar, kUnit, D) != CG_EINVAL) return 14;
  if (!strstr(cg_last_error(), "rule 3:")) return 15;
  memcpy(bad, kPar, sizeof bad);
  bad[6] = -2;
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, bad, kUnit, D) != CG_EINVAL) return 16;
  if (!strstr(cg_last_error(), "rule 6:")) return 17;
  memcpy(ubad, kUnit, sizeof ubad);
  ubad[4] = 2; /* 0 0 3 3 2: decreases */
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, ubad, D) != CG_EINVAL) return 18;
  if (!strstr(cg_last_error(), "rule 4:")) return 19;
  memcpy(bad, kPar, sizeof bad);
  bad[8] = 15; /* differs from rule 7 of the same unit */
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, bad, kUnit, D) != CG_EINVAL) return 20;
  if (!strstr(cg_last_error(), "rule 8:")) return 21;
  memcpy(bad, kPar, sizeof bad);
  bad[9] = 17; /* runs for ever, so 17 can drop */
  if (cg_admit_device(ctx, sp, ny, 0, WIDTH, NB, kDur, bad, kUnit, D) != CG_ERANGE) return 22;
  if (!strstr(cg_last_error(), "rule 9:")) return 23;
  if (cg_admit_per_node_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, A, NULL, 0) != CG_EINVAL) return 24;
  if (cg_admit_per_node_device(ctx, sp, ny, 0, WIDTH, NB, kDur, kPar, kUnit, A, rules, 3) != CG_EINVAL) return 25;
  if (cg_profile_kind(ctx, &kind) != CG_EINVAL) return 26; /* nothing readable yet */

  /* six hours before the 2026-03-08 spring-forward, at a non-aligned second */
  const int64_t t0 = 1772953200LL - 6 * 3600 + 17;
  static int32_t rows[NSPEC * NB];
  static int64_t totals[NB], nodes[16 * NB], peak[16];
  static int32_t bucket[16];
  for (int pass = 0; pass < 2; pass++) {
    CHECK(cg_admit_device(ctx, sp, ny, t0, WIDTH, NB, kDur, kPar, kUnit, pass ? A : D));
    CHECK(cg_profile_kind(ctx, &kind));
    printf("K %d\n", kind);
    CHECK(cg_profile_copy_rules(ctx, 0, NSPEC, rows));
    CHECK(cg_profile_copy_totals(ctx, totals));
    for (int r = 0; r < NSPEC; r++) {
      printf(pass ? "A" : "D");
      for (int b = 0; b < NB; b++) printf(" %d", rows[r * NB + b]);
      printf("\n");
    }
    printf(pass ? "T" : "S");
    for (int b = 0; b < NB; b++) printf(" %lld", (long long)totals[b]);
    printf("\n");
  }
  if (cg_profile_node_peaks(ctx, 0, 1, peak, bucket) != CG_EINVAL) return 27; /* no node matrix yet */

  if (rin.n_nodes > 16) return 28;
  CHECK(cg_admit_per_node_device(ctx, sp, ny, t0, WIDTH, NB, kDur, kPar, kUnit, D, rules, CG_EXCLUDE_NONE));
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
  /* an in-flight profile replaces it */
  CHECK(cg_inflight_device(ctx, sp, ny, t0, WIDTH, NB, kDur));
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
