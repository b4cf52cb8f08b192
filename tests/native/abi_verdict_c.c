/*
 * abi_verdict_c.c -- the fire-verdict entry points of the C-ABI
 * (include/cronsun_gpu.h) driven from plain C11 on a six-rule set:
 * cg_expand_verdicts_device with both argument structs, cg_result_copy_*,
 * cg_verdicts_device, cg_verdicts_copy, cg_verdicts_select_device,
 * cg_verdicts_selected_device, cg_verdicts_selected_copy_*, cg_verdict_times.
 * Test infrastructure: tests/test_abi_verdict_c.py compiles it with
 * `gcc -std=c11 -pedantic -Werror` and compares what it prints with the model.
 *
 *   abi_verdict_c <zoneinfo dir>      "K key values..." lines
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

static const char* kSpecs[] = {"*/10 * * * * *", "*/15 * * * * *", "@every 90s", "0 0 0 30 Feb ?", "0 * * * * *",
                               "7,30,45 * * * * *"};
#define NSPEC ((int)(sizeof kSpecs / sizeof kSpecs[0]))
#define HORIZON 1800
#define MAXE 4096
/* admission units {0,1} {2} {3} {4,5}; lock units (jobs) {0,1} {2,3} {4,5} */
static const int64_t kDur[NSPEC] = {25000, 25000, 180001, 0, 20000, 20000};
static const int64_t kPar[NSPEC] = {2, 2, 1, 1, 1, 1};
static const int32_t kUnit[NSPEC] = {0, 0, 3, 4, 7, 7};
static const int32_t kKind[NSPEC] = {CG_JOB_COMMON, CG_JOB_COMMON, CG_JOB_ALONE, CG_JOB_ALONE, CG_JOB_INTERVAL,
                                     CG_JOB_INTERVAL};
static const int64_t kAvg[NSPEC] = {25000, 25000, 180001, 180001, 20000, 20000};
static const int32_t kJob[NSPEC] = {0, 0, 1, 1, 2, 2};
static const uint8_t kContends[NSPEC] = {1, 1, 1, 1, 1, 0};

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
  if (CG_VERDICT_DROPPED != 1 || CG_VERDICT_SKIPPED != 2) return 5;
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
  printf("J rules %d\n", NSPEC);

  cg_ctx* ctx = NULL;
  int rc = cg_init(0, &ctx);
  if (rc == CG_ENODEV) {
    printf("NODEV %s\n", cg_last_error());
    cg_zone_free(ny);
    return 0;
  }
  CHECK(rc);
  cg_specs* sp;
  CHECK(cg_specs_upload_schedules(ctx, sched, NSPEC, &sp));

  const cg_admit_args admit = {kDur, kPar, kUnit};
  const cg_lock_args lock = {kKind, kAvg, kJob, kContends, 300};
  /* 15 minutes before the 2026-03-08 spring-forward, at a non-aligned second */
  const int64_t t0 = 1772953200LL - 900 + 17, t1 = t0 + HORIZON;
  int64_t n = -1, nsel = -1;
  const uint8_t* d_v = NULL;
  const int64_t *d_so = NULL, *d_st = NULL;
  static uint8_t v[MAXE];
  static int64_t off[NSPEC + 1], times[MAXE], sel_off[NSPEC + 1], sel_times[MAXE];

  /* the accessors before any call, and the refusals that come before any device work */
  if (cg_verdicts_device(ctx, &d_v, &n) != CG_EINVAL) return 7;
  if (cg_verdicts_copy(ctx, 0, 0, v) != CG_EINVAL) return 8;
  if (cg_verdicts_select_device(ctx, 1, 1, &nsel) != CG_EINVAL) return 9;
  if (cg_verdicts_selected_device(ctx, &d_so, &d_st, &nsel) != CG_EINVAL) return 10;
  if (cg_verdicts_selected_copy_offsets(ctx, sel_off) != CG_EINVAL) return 11;
  if (cg_verdicts_selected_copy_times(ctx, 0, 0, sel_times) != CG_EINVAL) return 12;
  if (cg_expand_verdicts_device(ctx, sp, ny, t0, t1, NULL, NULL, &n) != CG_EINVAL) return 13;
  if (cg_expand_verdicts_device(ctx, sp, ny, t1, t0, &admit, &lock, &n) != CG_EINVAL) return 14;
  if (cg_expand_verdicts_device(ctx, sp, ny, 0, CG_MAX_HORIZON + 1, &admit, NULL, &n) != CG_ERANGE) return 15;
  {
    cg_lock_args bad = lock;
    bad.lock_ttl = 1;
    if (cg_expand_verdicts_device(ctx, sp, ny, t0, t1, NULL, &bad, &n) != CG_EINVAL) return 16;
    int64_t par[NSPEC];
    memcpy(par, kPar, sizeof par);
    par[1] = 3; /* differs from rule 0 of the same unit */
    cg_admit_args abad = admit;
    abad.parallels = par;
    if (cg_expand_verdicts_device(ctx, sp, ny, t0, t1, &abad, NULL, &n) != CG_EINVAL) return 17;
    if (!strstr(cg_last_error(), "rule 1:")) return 18;
  }
  if (cg_verdicts_device(ctx, &d_v, &n) != CG_EINVAL) return 19; /* still nothing readable */

  CHECK(cg_expand_verdicts_device(ctx, sp, ny, t0, t1, &admit, &lock, &n));
  if (n < 1 || n > MAXE) return 20;
  int64_t n2 = -1;
  CHECK(cg_verdicts_device(ctx, &d_v, &n2));
  if (n2 != n || !d_v) return 21;
  CHECK(cg_result_copy_offsets(ctx, off));
  CHECK(cg_result_copy_times(ctx, 0, n, times));
  CHECK(cg_verdicts_copy(ctx, 0, n, v));
  if (cg_verdicts_copy(ctx, 1, n, v) != CG_EINVAL) return 22; /* past the end */
  printf("N %lld\n", (long long)n);
  for (int r = 0; r < NSPEC; r++) {
    printf("V");
    for (int64_t e = off[r]; e < off[r + 1]; e++) printf(" %lld:%d", (long long)times[e], v[e]);
    printf("\n");
  }
  if (cg_verdicts_selected_device(ctx, &d_so, &d_st, &nsel) != CG_EINVAL) return 23; /* no selection yet */
  if (cg_verdicts_select_device(ctx, 0, 0, &nsel) != CG_EINVAL) return 24;
  if (cg_verdicts_select_device(ctx, 4, 0, &nsel) != CG_EINVAL) return 25;
  if (cg_verdicts_select_device(ctx, 1, 2, &nsel) != CG_EINVAL) return 26;
  static const int kSel[3][2] = {{1, 1}, {2, 2}, {3, 0}};
  for (int i = 0; i < 3; i++) {
    CHECK(cg_verdicts_select_device(ctx, kSel[i][0], kSel[i][1], &nsel));
    if (nsel < 0 || nsel > n) return 27;
    int64_t nsel2 = -1;
    CHECK(cg_verdicts_selected_device(ctx, &d_so, &d_st, &nsel2));
    if (nsel2 != nsel || !d_so || !d_st) return 28;
    CHECK(cg_verdicts_selected_copy_offsets(ctx, sel_off));
    CHECK(cg_verdicts_selected_copy_times(ctx, 0, nsel, sel_times));
    printf("S %d %d %lld\n", kSel[i][0], kSel[i][1], (long long)nsel);
    for (int r = 0; r < NSPEC; r++) {
      printf("L");
      for (int64_t e = sel_off[r]; e < sel_off[r + 1]; e++) printf(" %lld", (long long)sel_times[e]);
      printf("\n");
    }
  }
  float ms[6];
  if (cg_verdict_times(ctx, ms, 6) != 6) return 29;
  /* a later expansion call replaces the result the bytes belong to */
  int64_t n3 = -1;
  CHECK(cg_expand_device(ctx, sp, ny, t0, t1, &n3));
  if (n3 != n) return 30;
  if (cg_verdicts_device(ctx, &d_v, &n2) != CG_EINVAL) return 31;
  if (cg_verdicts_selected_copy_offsets(ctx, sel_off) != CG_EINVAL) return 32;
  printf("OK\n");
  cg_specs_free(sp);
  cg_destroy(ctx);
  cg_zone_free(ny);
  return 0;
}
