/*
 * abi_inflight_c.c -- the in-flight profile entry points of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on a ten-rule set, in the
 * call order of the cgo stub's InFlight / InFlightPerNode / NodePeaks:
 * cg_inflight_device, cg_profile_kind, cg_profile_copy_rules,
 * cg_profile_copy_totals, cg_inflight_per_node_device, cg_profile_copy_nodes,
 * cg_profile_node_peaks.  Test infrastructure: tests/test_abi_inflight_c.py
 * compiles it with `gcc -std=c11 -pedantic -Werror` and compares what it
 * prints with the oracle.
 *
 *   abi_inflight_c <zoneinfo dir>      "K key values..." lines
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

static const char* kSpecs[] = {"0 */5 * * * *",  "0 30 9 * * 1-5", "*/10 * * * * *", "@daily",       "@every 90s",
                               "0 0 0 30 Feb ?", "0 30 2 * * *",   "@hourly",        "7,30,45 * * * * *", "@every 7s"};
#define NSPEC ((int)(sizeof kSpecs / sizeof kSpecs[0]))
#define WIDTH 1800
#define NB 24
/* ms per rule: none, under a second, around the width, hours, the largest */
static const int64_t kDur[NSPEC] = {0,       300,      1799999, 1800000, 1800001,
                                    7200000, 18000000, 1001,    INT64_MAX, 60000};

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
  if (CG_PROFILE_STARTS != 0 || CG_PROFILE_INFLIGHT != 1) return 5;
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

  cg_jobset* js;
  CHECK(cg_jobset_new(&js));
  const char* g1[] = {"n1", "n2", "n3"};
  const char* g2[] = {"n3", "n4"};
  CHECK(cg_jobset_add_group(js, "g1", g1, 3));
  CHECK(cg_jobset_add_group(js, "g2", g2, 2));
  for (int i = 0; i < NSPEC; i++) {
    char id[16];
    snprintf(id, sizeof id, "job%d", i);
    CHECK(cg_jobset_add_job(js, id, i == 7));
    const char* gids[] = {i % 2 ? "g1" : "g2"};
    const char* nids[] = {"n5"};
    const char* ex[] = {"n3"};
    CHECK(cg_jobset_add_rule(js, "r", gids, 1, nids, (size_t)(i % 3 == 0), ex, (size_t)(i % 4 == 0)));
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
  memcpy(bad, kDur, sizeof bad);
  bad[3] = -1;
  if (cg_inflight_device(ctx, sp, ny, 0, 0, NB, kDur) != CG_EINVAL) return 7;
  if (cg_inflight_device(ctx, sp, ny, 0, WIDTH, 4097, kDur) != CG_EINVAL) return 8;
  if (cg_inflight_device(ctx, sp, ny, 0, CG_MAX_HORIZON, 2, kDur) != CG_ERANGE) return 9;
  if (cg_inflight_device(ctx, sp, ny, 0, WIDTH, NB, NULL) != CG_EINVAL) return 10;
  if (cg_inflight_device(ctx, sp, ny, 0, WIDTH, NB, bad) != CG_EINVAL) return 11;
  if (!strstr(cg_last_error(), "rule 3:")) return 12;
  if (cg_profile_kind(ctx, &kind) != CG_EINVAL) return 13; /* nothing readable yet */

  /* six hours before the 2026-03-08 spring-forward, at a non-aligned second */
  const int64_t t0 = 1772953200LL - 6 * 3600 + 17;
  CHECK(cg_inflight_device(ctx, sp, ny, t0, WIDTH, NB, kDur));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  static int32_t rows[NSPEC * NB];
  static int64_t totals[NB], nodes[16 * NB], peak[16];
  static int32_t bucket[16];
  CHECK(cg_profile_copy_rules(ctx, 0, NSPEC, rows));
  CHECK(cg_profile_copy_totals(ctx, totals));
  if (cg_profile_node_peaks(ctx, 0, 1, peak, bucket) != CG_EINVAL) return 14; /* no node matrix yet */
  for (int r = 0; r < NSPEC; r++) {
    printf("R");
    for (int b = 0; b < NB; b++) printf(" %d", rows[r * NB + b]);
    printf("\n");
  }
  printf("S");
  for (int b = 0; b < NB; b++) printf(" %lld", (long long)totals[b]);
  printf("\n");

  if (rin.n_nodes > 16) return 15;
  CHECK(cg_inflight_per_node_device(ctx, sp, ny, t0, WIDTH, NB, kDur, rules, CG_EXCLUDE_NONE));
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
  /* a start profile replaces it, and its peaks are served the same way */
  CHECK(cg_profile_per_node_device(ctx, sp, ny, t0, WIDTH, NB, rules, CG_EXCLUDE_NONE));
  CHECK(cg_profile_kind(ctx, &kind));
  printf("K %d\n", kind);
  CHECK(cg_profile_node_peaks(ctx, 1, 2, peak, bucket));
  printf("Q %lld %d %lld %d\n", (long long)peak[0], bucket[0], (long long)peak[1], bucket[1]);
  printf("OK\n");
  cg_rules_free(rules);
  cg_specs_free(sp);
  cg_destroy(ctx);
  cg_jobset_free(js);
  cg_zone_free(ny);
  return 0;
}
