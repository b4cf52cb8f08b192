/*
 * abi_top_rules_c.c -- the top-rules entry points of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on the ten-rule, five-node
 * set of abi_inflight_c.c, in the call order of the cgo stub's TopRules /
 * TopRulesBucket: cg_inflight_per_node_device, cg_profile_top_rules_nodes
 * (peak buckets, then explicit ones), cg_profile_top_rules_copy,
 * cg_profile_top_rules_device, cg_profile_top_rules_times,
 * cg_profile_top_rules_bucket.  Test infrastructure:
 * tests/test_abi_top_rules_c.py compiles it with `gcc -std=c11 -pedantic
 * -Werror` and compares what it prints with the model.
 *
 *   abi_top_rules_c <zoneinfo dir>      "K key values..." lines
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
#define K 3
#define MAXN 16
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

static int32_t rule[MAXN * CG_TOP_RULES_MAX], cnt[MAXN * CG_TOP_RULES_MAX];
static int32_t n_listed[MAXN], n_contrib[MAXN], bucket[MAXN];

/* rows [0, rows) of the readable result, k columns, under the line key */
static int print_rows(cg_ctx* ctx, const char* key, int rows, int k) {
  CHECK(cg_profile_top_rules_copy(ctx, 0, rows, rule, cnt, n_listed, n_contrib, bucket));
  for (int n = 0; n < rows; n++) {
    printf("%s %d %d %d %d", key, n, bucket[n], n_contrib[n], n_listed[n]);
    for (int i = 0; i < k; i++) printf(" %d:%d", rule[n * k + i], cnt[n * k + i]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (cg_abi_version() != CG_ABI_VERSION) return 4;
  if (CG_TOP_RULES_MAX != 64) return 5;
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
  if (rin.n_nodes > MAXN) return 7;
  const int N = rin.n_nodes;
  cg_specs* sp;
  CHECK(cg_specs_upload_schedules(ctx, sched, NSPEC, &sp));
  cg_rules* rules;
  CHECK(cg_rules_upload(ctx, &rin, &rules));

  /* nothing readable yet */
  if (cg_profile_top_rules_nodes(ctx, K, NULL) != CG_EINVAL) return 8;
  if (cg_profile_top_rules_bucket(ctx, 0, K) != CG_EINVAL) return 9;
  if (cg_profile_top_rules_copy(ctx, 0, 0, NULL, NULL, NULL, NULL, NULL) != CG_EINVAL) return 10;

  const int64_t t0 = 1772953200LL - 6 * 3600 + 17;
  /* a profile without a node matrix: the cluster-wide row works, the nodes do not */
  CHECK(cg_inflight_device(ctx, sp, ny, t0, WIDTH, NB, kDur));
  if (cg_profile_top_rules_nodes(ctx, K, NULL) != CG_EINVAL) return 11;
  CHECK(cg_profile_top_rules_bucket(ctx, NB - 1, CG_TOP_RULES_MAX));
  if (print_rows(ctx, "C", 1, CG_TOP_RULES_MAX)) return 1;

  CHECK(cg_inflight_per_node_device(ctx, sp, ny, t0, WIDTH, NB, kDur, rules, CG_EXCLUDE_NONE));
  if (cg_profile_top_rules_device(ctx, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != CG_EINVAL)
    return 12; /* the profile call dropped the list */
  CHECK(cg_profile_top_rules_nodes(ctx, K, NULL)); /* each node at its peak */
  if (print_rows(ctx, "P", N, K)) return 1;

  /* refusals leave that result readable */
  int32_t at[MAXN];
  for (int n = 0; n < N; n++) at[n] = (5 * n + 3) % NB;
  if (cg_profile_top_rules_nodes(ctx, 0, at) != CG_EINVAL) return 13;
  if (cg_profile_top_rules_nodes(ctx, CG_TOP_RULES_MAX + 1, at) != CG_EINVAL) return 14;
  at[2] = NB;
  if (cg_profile_top_rules_nodes(ctx, K, at) != CG_EINVAL) return 15;
  if (!strstr(cg_last_error(), "node 2:")) return 16;
  at[2] = (5 * 2 + 3) % NB;
  if (cg_profile_top_rules_bucket(ctx, -1, K) != CG_EINVAL) return 17;
  if (cg_profile_top_rules_copy(ctx, 1, N, rule, cnt, NULL, NULL, NULL) != CG_EINVAL) return 18;
  const int32_t *d_rule = NULL, *d_cnt = NULL;
  int32_t rows = -1, k = -1;
  CHECK(cg_profile_top_rules_device(ctx, &d_rule, &d_cnt, NULL, NULL, NULL, &rows, &k));
  if (!d_rule || !d_cnt || rows != N || k != K) return 19;
  if (print_rows(ctx, "Q", N, K)) return 1; /* the same lines as P */

  CHECK(cg_profile_top_rules_nodes(ctx, K, at));
  if (print_rows(ctx, "B", N, K)) return 1;
  float ms[3] = {-1.f, -1.f, -1.f};
  if (cg_profile_top_rules_times(ctx, ms, 3) != 3) return 20;
  printf("T %d\n", (int)ms[2]); /* chunks: one per node */

  CHECK(cg_profile_top_rules_bucket(ctx, 0, 2));
  if (print_rows(ctx, "D", 1, 2)) return 1;
  printf("OK\n");
  cg_rules_free(rules);
  cg_specs_free(sp);
  cg_destroy(ctx);
  cg_jobset_free(js);
  cg_zone_free(ny);
  return 0;
}
