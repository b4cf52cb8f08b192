/*
 * cronsun_gpu.h -- C-ABI of the MI355X fire-time expansion engine for
 * cronsun's scheduling path (library: cronsun_amd/libcronsun_gpu.so).
 *
 * This is the boundary a Go cgo package `node/cron/gpu` binds (see
 * INTEGRATION.md).  Plain pointers and sizes only; no C++ or torch types.
 * Every entry point names the reference interface it replaces
 * (paths relative to qlchan/cronsun).
 *
 * Conventions
 *   - Return value: CG_OK (0) or a negative CG_E* code; cg_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - Times are int64 unix seconds.  Go's zero time.Time{} (the "never fires"
 *     result of Schedule.Next) is CG_ZERO_TIME = -62135596800.
 *   - Input buffers are owned by the caller and only read during the call;
 *     nothing is retained (cgo rule: Go memory is never kept).
 *   - A cg_ctx owns one HIP device, its stream and its device buffers.  Calls
 *     on one ctx are serialised internally; calls block the calling thread.
 *   - There is no CPU fallback: compute entry points fail with CG_ENODEV
 *     when no MI355X (gfx950) device is usable.
 */
#ifndef CRONSUN_GPU_H
#define CRONSUN_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cg_rules_in.rule_key (Job.Cmds' Job.ID+Rule.ID map key)
 * 3: time-ordered per-node gather (cg_comm_gather_node_csr on time-ordered
 *    results, cg_node_csr_merge_ranks), cg_comm_gather_plan */
#define CG_ABI_VERSION 3

#define CG_OK 0
#define CG_EINVAL (-1)    /* bad argument */
#define CG_ENOMEM (-2)    /* host or device allocation failed */
#define CG_EHIP (-3)      /* HIP runtime error */
#define CG_ECAPACITY (-4) /* output buffer too small; required size reported */
#define CG_EPARSE (-5)    /* spec did not parse; message via cg_last_error */
#define CG_ERANGE (-6)    /* time range/horizon outside supported bounds */
#define CG_ENODEV (-7)    /* no usable gfx950 device */
#define CG_EPANIC (-8)    /* input on which the reference Go code panics */

#define CG_ZERO_TIME (-62135596800LL)

/* ParseOption bits -- node/cron/parser.go:17-26 */
#define CG_PARSE_SECOND 1
#define CG_PARSE_MINUTE 2
#define CG_PARSE_HOUR 4
#define CG_PARSE_DOM 8
#define CG_PARSE_MONTH 16
#define CG_PARSE_DOW 32
#define CG_PARSE_DOW_OPTIONAL 64
#define CG_PARSE_DESCRIPTOR 128
/* defaultParser, parser.go:171-173 (cron.Parse) */
#define CG_PARSE_DEFAULT (1 | 2 | 4 | 8 | 16 | 64 | 128)
/* standardParser, parser.go:155-157 (cron.ParseStandard) */
#define CG_PARSE_STANDARD (2 | 4 | 8 | 16 | 32 | 128)

#define CG_STAR_BIT (1ULL << 63) /* spec.go:48-51 */

/* A parsed cron.Schedule: *SpecSchedule (spec.go:7-9) or
 * ConstantDelaySchedule (constantdelay.go:7-9). */
typedef struct {
  int32_t kind; /* 0 = SpecSchedule, 1 = ConstantDelaySchedule */
  int32_t reserved;
  uint64_t second, minute, hour, dom, month, dow; /* SpecSchedule fields */
  int64_t delay_ns;                               /* ConstantDelaySchedule.Delay */
} cg_schedule;

typedef struct cg_ctx cg_ctx;
typedef struct cg_zone cg_zone;
typedef struct cg_specs cg_specs;
typedef struct cg_jobset cg_jobset;

/* ---------------------------------------------------------------- misc --- */
int cg_abi_version(void);
const char* cg_last_error(void);
/* number of gfx950 devices visible (0 on a host without one) */
int cg_device_count(void);
/* Build flags of the loaded library (instrumentation; no reference
 * counterpart).  CG_BUILD_DIAG: the diagnostic build (`make diag`), whose
 * writer honours probe/variant environment switches that replace or drop
 * output stores -- never a production or benchmark library. */
#define CG_BUILD_DIAG 1
int cg_build_info(void);

/* ------------------------------------------------------ parse (host) --- */
/* Parser{options}.Parse(spec) -- parser.go:78-136; cron.Parse is options =
 * CG_PARSE_DEFAULT (parser.go:181-183), cron.ParseStandard CG_PARSE_STANDARD
 * (parser.go:167-169).  On error returns CG_EPARSE and copies Go's message
 * into err (NUL-terminated, truncated to err_cap) and cg_last_error(). */
int cg_parse(int options, const char* spec, size_t len, cg_schedule* out, char* err,
             size_t err_cap);
/* Batch form: n specs, status[i] = 0 or a CG_E* code. */
int cg_parse_batch(int options, const char* const* specs, const size_t* lens, size_t n,
                   cg_schedule* out, int32_t* status, int nthreads);
/* Parser internals, exposed for the reference's parser KATs
 * (parser_test.go TestRange/TestField/TestBits): getRange (parser.go:204-267),
 * getField (parser.go:188-199), getBits (parser.go:293-306).  names: 0 none,
 * 1 month names, 2 day-of-week names. */
int cg_get_range(const char* expr, size_t len, unsigned min, unsigned max, int names,
                 uint64_t* bits, char* err, size_t err_cap);
int cg_get_field(const char* expr, size_t len, unsigned min, unsigned max, int names,
                 uint64_t* bits, char* err, size_t err_cap);
uint64_t cg_get_bits(unsigned min, unsigned max, unsigned step);
/* Every(d).Delay -- constantdelay.go:14-21 */
int64_t cg_every(int64_t duration_ns);
/* time.ParseDuration (used by "@every", parser.go:368-373) */
int cg_parse_duration(const char* s, size_t len, int64_t* out_ns);

/* ------------------------------------------------------------- zones --- */
/* time.LoadLocationFromTZData (TZif v1-v4 incl. the POSIX footer). */
int cg_zone_from_tzif(const uint8_t* data, size_t len, cg_zone** out);
/* time.FixedZone("", offset_sec) */
int cg_zone_fixed(int32_t offset_sec, cg_zone** out);
/* time.UTC */
int cg_zone_utc(cg_zone** out);
void cg_zone_free(cg_zone* z);
/* Location.lookup(unix).offset (host, for inspection/tests) */
int cg_zone_offset(const cg_zone* z, int64_t unix_sec, int32_t* offset_sec);
/* The flat breakpoint table the kernels use for [lo, hi]: when[0] is
 * INT64_MIN, then every instant in (lo, hi] where the offset changes.
 * Returns the entry count (writes at most cap). */
int cg_zone_table(const cg_zone* z, int64_t lo, int64_t hi, int64_t* when, int32_t* off,
                  int cap);

/* ----------------------------------------------------------- context --- */
int cg_init(int device, cg_ctx** out);
void cg_destroy(cg_ctx* ctx);
/* wait for all work queued on the ctx's stream */
int cg_sync(cg_ctx* ctx);

/* -------------------------------------------------- specs (HBM SoA) --- */
/* SoA upload of SpecSchedule/ConstantDelaySchedule values (spec.go:7-9,
 * constantdelay.go:7-9).  delay_ns[i] > 0 marks rule i as @every; the mask
 * arrays are then ignored for it. Any array may be NULL if unused. */
typedef struct {
  const uint64_t* second;
  const uint64_t* minute;
  const uint64_t* hour;
  const uint64_t* dom;
  const uint64_t* month;
  const uint64_t* dow;
  const int64_t* delay_ns;
} cg_spec_soa;
int cg_specs_upload(cg_ctx* ctx, const cg_spec_soa* soa, size_t n_rules, cg_specs** out);
int cg_specs_upload_schedules(cg_ctx* ctx, const cg_schedule* s, size_t n_rules,
                              cg_specs** out);
/* rules [first, first+count) of an uploaded set, as a view (no copy) -- used
 * to shard rules by job-ID range across ranks.  Free views with
 * cg_specs_free as well; the view must not outlive its parent. */
int cg_specs_slice(cg_specs* specs, size_t first, size_t count, cg_specs** out);
size_t cg_specs_count(const cg_specs* specs);
void cg_specs_free(cg_specs* specs);

/* --------------------------------------------------------- Next() ------ */
/* out[i] = Schedule.Next(t_in[i]) for rule i, evaluated in zone z
 * (spec.go:55-145, constantdelay.go:25-27).  Host arrays of n = rule count.
 * Never-firing specs give CG_ZERO_TIME; a rule whose Next never returns
 * (AddDate stuck on a skipped local day) gives CG_NO_PROGRESS_TIME.  Replaces per-entry calls in
 * Cron.run (cron.go:212-215, 242-243) and Cmd.lockTtl (job.go:196-197). */
int cg_next_batch(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, const int64_t* t_in,
                  int64_t* t_out);

/* ---------------------------------------------------- Cmd.lockTtl() ---- */
/* ttl_out[i] = Cmd.lockTtl() (job.go:194-233) for rule i at time now[i]:
 *   prev = Next(now); ttl = Next(prev).Sub(prev) / Second (saturating);
 *   ttl == 0 -> 0 (lock() treats the rule as invalid, job.go:246-248);
 *   kind[i] == CG_JOB_INTERVAL -> clamp(ttl - 2, 1, lock_ttl);
 *   otherwise ttl -= cost when ttl >= cost, cost = avg_time_ms[i] / 1e3 in
 *   Go int64 arithmetic (so the ceiling at job.go:214 only fires for a
 *   negative AvgTime), then clamp to [2, lock_ttl].
 * kind = Job.Kind (job.go:30-34), avg_time_ms = Job.AvgTime,
 * lock_ttl = conf.Config.LockTtl (conf.go:136-138 defaults it to 300).
 * A rule whose Next never returns gets CG_NO_PROGRESS_TIME.  Host arrays of
 * n = rule count.  Replaces the per-Cmd call in newLock (job.go:235-241). */
#define CG_JOB_COMMON 0
#define CG_JOB_ALONE 1
#define CG_JOB_INTERVAL 2
#define CG_NO_PROGRESS_TIME (INT64_MIN + 1)
int cg_lock_ttl_batch(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, const int64_t* now,
                      const int32_t* kind, const int64_t* avg_time_ms, int64_t lock_ttl,
                      int64_t* ttl_out);

/* ------------------------------------------------------- dispatcher ---- */
/* The state of Cron.run (node/cron/cron.go:210-275) resident in HBM.  Entries
 * are slots 0..count-1 (the caller maps Entry IDs, cron.go:17-27 `indexes`,
 * to slots).  Each slot holds a schedule, Next and Prev (unix seconds;
 * CG_ZERO_TIME = zero time).
 *
 *   cg_dispatcher_new        run() start: Next = Schedule.Next(now) for every
 *                            entry of specs (cron.go:212-215); Prev = zero.
 *   cg_dispatcher_effective  entries[0].Next after sort.Sort(byTime)
 *                            (cron.go:220-230): the earliest non-zero Next, or
 *                            CG_ZERO_TIME when none (the loop then sleeps
 *                            ten years).
 *   cg_dispatcher_fire       the timer fired at `now` >= effective
 *                            (cron.go:234-244): every entry whose Next ==
 *                            effective is due; its Prev = Next and
 *                            Next = Schedule.Next(now).  Returns the due count
 *                            and the next effective time.
 *   cg_dispatcher_due        the last wake's due slots, ascending (the
 *                            reference runs them in byTime order, which is
 *                            unordered among equal Next values).
 *   cg_dispatcher_set        add or replace entries (cron.go:246-252,
 *                            125-142): slot idx[j] gets schedule s[j],
 *                            Next = Schedule.Next(now), Prev = zero.  Slots
 *                            past the current count extend it; skipped slots
 *                            stay empty.
 *   cg_dispatcher_remove     DelJob (cron.go:149-164, 254-262): the slot is
 *                            emptied and never fires.
 *   cg_dispatcher_snapshot   Entries() (cron.go:166-174, 296-308): Next, Prev
 *                            and liveness per slot (any pointer may be NULL).
 * A schedule whose Next never returns (the reference loop then blocks
 * forever) makes the call fail with CG_ERANGE naming the lowest such slot.
 * Such a failed new / fire / set has otherwise taken effect: every other
 * entry of the call is placed or advanced exactly, the due list of a failed
 * fire is readable with cg_dispatcher_due, and the effective time is the
 * minimum over the other entries.  The stuck slot stays live with Next =
 * CG_NO_PROGRESS_TIME (a failed fire has set its Prev), never fires and never
 * holds the effective time until it is replaced or removed.
 * cg_dispatcher_new writes *out once the table is built: a failure before
 * that (bad arguments, no memory, `now` out of range) leaves *out as the
 * caller set it, and on this CG_ERANGE *out holds the dispatcher just
 * described.  Set *out to NULL before the call; when it is not NULL after a
 * failed one, the caller must free it with cg_dispatcher_free (or, after this
 * CG_ERANGE, may go on with it). */
typedef struct cg_dispatcher cg_dispatcher;
int cg_dispatcher_new(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t now,
                      cg_dispatcher** out);
void cg_dispatcher_free(cg_dispatcher* d);
int64_t cg_dispatcher_count(const cg_dispatcher* d);
int cg_dispatcher_effective(const cg_dispatcher* d, int64_t* effective);
int cg_dispatcher_fire(cg_dispatcher* d, int64_t now, int64_t* n_due, int64_t* effective);
int cg_dispatcher_due(const cg_dispatcher* d, int64_t first, int64_t count, int32_t* out);
/* the due list in HBM (valid until the next call on d) */
int cg_dispatcher_due_device(const cg_dispatcher* d, const int32_t** due, int64_t* n_due);
int cg_dispatcher_set(cg_dispatcher* d, const int64_t* idx, const cg_schedule* s, size_t k,
                      int64_t now);
int cg_dispatcher_remove(cg_dispatcher* d, const int64_t* idx, size_t k);
int cg_dispatcher_snapshot(const cg_dispatcher* d, int64_t* next, int64_t* prev, uint8_t* live);

/* --------------------------------------------------------- expansion --- */
/* counts[r] = number of fires of rule r in (t0, t1] (the expansion's count
 * pass alone: plan + k_count + scan; no times are written), *total = their
 * sum.  The cheap pass that balances job-ID-range shards by estimated events
 * (SURVEY.md §8e).  Leaves no expansion result behind. */
int cg_count(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t t1,
             int64_t* counts, int64_t* total);

/* Fire times of every rule over (t0, t1]: for each rule,
 *   t = t0; loop { t = Next(t); if t.IsZero() || t > t1 break; emit t }
 * i.e. the reference Next loop, batched.  Output is a rule-major CSR:
 *   offsets[R+1] (int64), times[offsets[R]] (int64, ascending per rule).
 * The reference loop takes any horizon (its only limit is Next's own: no
 * match within five calendar years of t returns the zero time and ends the
 * rule, spec.go:70-76 -- reproduced).  Internally the horizon is cut into
 * closed-form segments of <= 30 days, each continuing from the previous
 * segment's last fire; t1 - t0 may be up to CG_MAX_HORIZON seconds (40
 * years; CG_ERANGE beyond, or if a zone's transitions need more than 1024
 * segments). */
#define CG_MAX_HORIZON (14610LL * 86400)
typedef struct {
  int64_t* offsets;  /* [R+1], caller-allocated (may be NULL) */
  int64_t* times;    /* [times_cap], caller-allocated (may be NULL) */
  int64_t times_cap;
  int64_t n_events;  /* out: total events (always set, also on CG_ECAPACITY) */
} cg_csr;
int cg_expand(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t t1,
              cg_csr* out);

/* Device-resident variant: runs the whole expansion on the ctx's stream and
 * leaves offsets/times in device memory owned by the ctx (valid until the next
 * expansion call on this ctx).  *n_events is set.  Used for benchmarks and by
 * multi-GPU drivers that keep results in HBM. */
int cg_expand_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                     int64_t t1, int64_t* n_events);
/* Pipelined variant for back-to-back calls (a scheduler's tick loop over
 * consecutive windows, cron.go:212-215 per tick): enqueues the expansion and
 * returns without waiting.  The count/scan of a call overlap the previous
 * call's output write; each call's plan is staged without a stream sync, so
 * T0 may move every call.  Needs the output capacity left by an earlier
 * cg_expand_device large enough for every call's result: a call that would
 * exceed it writes nothing and cg_expand_wait returns CG_ECAPACITY.  Results
 * and errors are known only after cg_expand_wait, which waits for every
 * call issued since the last wait, returns the first error among them (a
 * rule whose reference loop never ends: CG_ERANGE, as cg_expand_device), and
 * sets *n_events of the last call, whose result the accessors below then
 * read.
 * Output buffers: consecutive calls alternate between two writer streams and
 * two output buffers (the ctx's own, which the synchronous calls write, and a
 * second of the same capacity), so two calls' writers run side by side and
 * the stores do not pause while one ends and the next starts.  The second
 * buffer costs one more result-sized allocation and is taken only when that
 * capacity is at most half of the device memory free at the moment (checked by
 * a call made with nothing pending, and again after a synchronous call grew
 * the capacity); where it does not fit, its allocation fails, or
 * cg_set_async_overlap(ctx, 0) was called, every call writes the one buffer on
 * the ctx stream, as a synchronous call does.  Either way, after the wait only
 * the LAST call's result is readable (earlier calls leave nothing readable):
 * cg_result_device returns the buffer that call wrote, which differs from call
 * to call -- its pointers are valid until the next expansion call, not beyond.
 * cg_last_kernel_times [3] = the mean over those calls of the writer time:
 * from the writer's start to its end, or, when the previous call's writer
 * still ran on the other stream at that start, from that writer's end to this
 * one's (0 if this one ended first).  These per-call intervals never overlap,
 * so in a pipelined run [3] reads as completion-to-completion time per call.
 * A returned error may belong to any call since the previous wait (its
 * message names the rule or the sizes).  *n_events is always set (0 when no
 * asynchronous call was made).  While calls are pending the result accessors
 * below refuse with CG_EINVAL.  A synchronous expansion (cg_expand,
 * cg_expand_device, cg_count, cg_expand_per_node*) made while calls are
 * pending drains them and discards their results and errors: call
 * cg_expand_wait first to observe them. */
int cg_expand_device_async(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                           int64_t t1);
int cg_expand_wait(cg_ctx* ctx, int64_t* n_events);
/* on != 0 (default): pipelined calls alternate between two writer streams and
 * output buffers when the second buffer fits (above); 0: one stream, one
 * buffer, and the second buffer is freed.  Takes effect from the next
 * cg_expand_device_async made with nothing pending; CG_EINVAL while calls are
 * pending.  Results are the same either way.  (No reference counterpart: a
 * memory-for-throughput knob.) */
int cg_set_async_overlap(cg_ctx* ctx, int on);
/* device pointers of the last device-resident result (valid until the next
 * expansion call on this ctx; after pipelined calls d_times is the buffer the
 * last call wrote) */
int cg_result_device(cg_ctx* ctx, const int64_t** d_offsets, const int64_t** d_times,
                     int64_t* n_events);
/* copy [first, first+count) of the last result's times to host */
int cg_result_copy_times(cg_ctx* ctx, int64_t first, int64_t count, int64_t* host_out);
int cg_result_copy_offsets(cg_ctx* ctx, int64_t* host_offsets /* [R+1] */);

/* Per-kernel device time of the last expansion (ms, HIP events on the ctx
 * stream): [0] count, [1] scan, [2] block map, [3] write (closed form; after
 * pipelined calls see cg_expand_device_async),
 * [4] write (walk), [5] offsets; of the last per-node call: [6] rule->node
 * join, [7] transpose (when the join is rebuilt) + segment records + per-node
 * offsets, [8] per-node write; [12] the last time-order pass; of the last
 * dispatcher wake: [9] scan, [10] due compaction, [11] advance; [13] the last
 * cg_dispatcher_fanout; of the last profile call (starts or in flight): [14] rule matrix, [15]
 * walked runs, [16] totals, [17] join + transpose (when rebuilt), [18] node
 * matrix; of the last admission or lock profile: [19] the pass that zeroes the
 * rewritten rows, [20] the admission unit walk, [21] the lock unit walk; of
 * the last running profile (CG_PROFILE_RUNNING / CG_PROFILE_LOCK_RUNNING): [22]
 * the prefix sum along the rewritten rows (23 entries in all).  n = entries
 * written. */
int cg_last_kernel_times(cg_ctx* ctx, float* ms, int n);
/* Expansion phase timing: 2 (default) = a HIP event between every phase;
 * 1 = events around k_write_cf only ([3]; [0..2], [4], [5] read -1).  Events
 * recorded between kernels leave the GPU idle for several us each, so
 * throughput measurements use 1.  (No reference counterpart: instrumentation.) */
int cg_set_phase_timing(cg_ctx* ctx, int level);

/* Order-sensitive checksum of a device array on the ctx's device
 * (instrumentation for integrity and parity checks; no reference
 * counterpart): sum over i < n of mix(first_index + i, v[i] + add) mod 2^64,
 * v = int64 (elem_bytes 8) or int32 (elem_bytes 4, sign-extended to 64 bits).
 * Both sums are taken mod 2^64 -- first_index + i and v[i] + add wrap like
 * unsigned 64-bit integers, for any int64 first_index and add -- and
 *   mix(p, x) = fin(x XOR fin(p * 0x9E3779B97F4A7C15 mod 2^64)),
 * fin = the splitmix64 finaliser (shifts 30, 27, 31; multipliers
 * 0xBF58476D1CE4E5B9, 0x94D049BB133111EB).
 * Checksums of consecutive ranges add up (mod 2^64), so a shard's output
 * (first_index = its global base) can be compared with its range of another
 * result. */
int cg_checksum_device(cg_ctx* ctx, const void* d_ptr, int64_t n, int elem_bytes,
                       int64_t first_index, int64_t add, uint64_t* out);
/* Integrity helpers for benchmarks and tests (no reference counterpart):
 * fill `bytes` of a device buffer with one byte value (e.g. poison an output
 * before timed runs), and count the int64/int32 elements equal to `value`
 * (e.g. poison a later run left unwritten).  `value` is compared as an int64:
 * with elem_bytes 4 a value outside the int32 range equals no element, the
 * count is 0 (it is never truncated to its low 32 bits). */
int cg_fill_device(cg_ctx* ctx, void* d_ptr, int64_t bytes, int byte_value);
int cg_count_value_device(cg_ctx* ctx, const void* d_ptr, int64_t n, int elem_bytes, int64_t value,
                          int64_t* count);
/* The store ceiling of this device (instrumentation; no reference
 * counterpart): the rate at which `bytes` (a multiple of 16) of the device
 * buffer d_ptr can be written, measured on the ctx stream with HIP events as
 * the mean over `reps` launches after one warm-up, for three fills:
 *   ms[0]  k_fill_stream, 16 B per lane nontemporal stores, a grid-stride
 *          loop over the whole buffer at full occupancy (one launch);
 *   ms[1]  the same with plain stores;
 *   ms[2]  hipMemsetAsync of the same bytes.
 * The output-bound kernels' roofline fractions are also reported against the
 * fastest of the three.  The buffer's contents are overwritten. */
int cg_fill_rate_device(cg_ctx* ctx, void* d_ptr, int64_t bytes, int reps, float* ms /* [3] */);

/* --------------------------------------------- rule -> node resolution --- */
/* Integer-interned jobs/groups (host interns string IDs; see cg_jobset_*).
 * Resolution modes:
 *   CG_EXCLUDE_NONE       reference scheduling semantics, Job.Cmds/IsRunOn
 *                         (job.go:591-630): ExcludeNodeIDs has no effect (the
 *                         inner-loop `continue`, job.go:598-602); Pause => none.
 *   CG_EXCLUDE_RULE       per-rule exclusion N_r \ E_r; Pause => none.
 *   CG_EXCLUDE_CUMULATIVE web/job.go:222-257 GetJobNodes: N_r \ U_{q<=r} E_q
 *                         over the job's rules in order; Pause => none. */
#define CG_EXCLUDE_NONE 0
#define CG_EXCLUDE_RULE 1
#define CG_EXCLUDE_CUMULATIVE 2
typedef struct {
  int32_t n_nodes, n_groups, n_rules, n_jobs;
  const int64_t* group_off;     /* [G+1] group -> node CSR (Group.NodeIDs, group.go:17-22) */
  const int32_t* group_nodes;
  const uint8_t* group_exists;  /* [G] 0 = gid referenced but absent from the groups map */
  const int32_t* rule_job;      /* [R] owning job; a job's rules are contiguous, in order */
  const int64_t* nid_off;       /* [R+1] JobRule.NodeIDs */
  const int32_t* nids;
  const int64_t* gid_off;       /* [R+1] JobRule.GroupIDs */
  const int32_t* gids;
  const int64_t* ex_off;        /* [R+1] JobRule.ExcludeNodeIDs */
  const int32_t* ex;
  const uint8_t* job_pause;     /* [J] Job.Pause */
  /* [R] or NULL: the rule's Cmd key (job.go:130-132 Cmd.GetID() = Job.ID +
   * Rule.ID), interned to any int32 such that two rules OF THE SAME JOB have
   * equal values exactly when their Rule.IDs are equal.  Job.Cmds keeps one
   * Cmd per key -- `cmds[cmd.GetID()] = cmd` (job.go:604-609): the LAST
   * included rule of the job with that key -- and the node's Cron replaces an
   * entry by ID (node/node.go:209-211, node/cron/cron.go:131-135).  So in
   * every mode the pair (r, n) is dropped when a later rule of r's job with
   * the same key is also scheduled on n (under the same mode: RULE and
   * CUMULATIVE test the later rule with their own exclusion).  Keys are only
   * compared within a job: equal Job.ID+Rule.ID strings of DIFFERENT jobs
   * ("a"+"bc", "ab"+"c") replace each other in the reference in the random
   * order of GetJobs' map, so both are kept here.  NULL: every rule is its
   * own key (the caller guarantees distinct Rule.IDs within a job).
   * cg_jobset_rules fills it from the Rule.IDs. */
  const int32_t* rule_key;
} cg_rules_in;
/* Limits of a rule set.  nids, gids and group_nodes must be in range
 * (CG_EINVAL otherwise); an ExcludeNodeID may be any id in [0, 2^31 - 1] --
 * one at or past n_nodes excludes nothing.  The join keeps a rule's node set
 * as a bitmap in the 64 KiB of LDS one wave may ask for, so a rule set has at
 * most 524288 nodes, and at most 262144 when some job repeats a Cmd key
 * (rule_key given and equal for two rules of one job: the later rules' sets
 * take a second bitmap).  rule_key that repeats no key inside a job counts as
 * NULL.  One node more and every call that builds the join -- cg_rule_nodes,
 * cg_expand_per_node*, cg_profile_per_node_device, cg_dispatcher_bind_rules,
 * cg_dispatcher_patch_rules for its patch -- fails with CG_ERANGE before any
 * kernel runs.  After such a refusal nothing of the refused set is bound or
 * cached: a dispatcher that called bind_rules is unbound (its fan-out is
 * CG_EINVAL until a bind succeeds; a refused patch leaves the bound join as
 * it was); a refused per-node call leaves no readable per-node result; it
 * and a refused profile call leave no per-node join cache, so the next
 * per-node call on any rule set builds its own join; a refused cg_rule_nodes
 * leaves an earlier per-node result and its cache as they were. */

/* Per-node fire lists: for every node n, the (time, rule) events of the rules
 * scheduled on n (per `mode`), rule-major in ascending rule index, times
 * ascending within a rule.  Output CSR: node_off[N+1], time[], rule[].
 * Replaces every node's Node.loadJobs -> addJob -> Job.Cmds filter
 * (node/node.go:121-158) plus its Cron entries' Next loop. */
typedef struct {
  int64_t* node_off;  /* [N+1] caller-allocated (may be NULL) */
  int64_t* time;      /* [cap] */
  int32_t* rule;      /* [cap] */
  int64_t cap;
  int64_t n_events;   /* out */
  int64_t nnz;        /* out: sum over rules of |nodes(rule)| */
} cg_node_csr;
int cg_expand_per_node(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                       int64_t t1, const cg_rules_in* rules, int mode, cg_node_csr* out);
/* device-resident variant (bench / multi-GPU); results stay in ctx memory */
int cg_expand_per_node_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                              int64_t t1, const cg_rules_in* rules, int mode,
                              int64_t* n_events, int64_t* nnz);
/* device pointers of the last per-node result */
int cg_node_result_device(cg_ctx* ctx, const int64_t** d_node_off, const int64_t** d_time,
                          const int32_t** d_rule, int64_t* n_events);
/* The rule bands of the last successful synchronous per-node call
 * (cg_expand_per_node*), which pipelined windows reuse: every node's list is
 * written in K = ceil(n_rules / B) segments of B consecutive rules (B >=
 * 32768 unless a band would hold more than 2^30 fires).  Read-only, no device
 * work; either pointer may be NULL.  CG_EINVAL before the first such call. */
int cg_node_result_bands(cg_ctx* ctx, int32_t* rules_per_band, int32_t* n_bands);
/* Reorder every node's list of the last per-node result by (time, rule), in
 * device memory: the order the node's scheduler keeps its entries in
 * (Cron.run's sort.Sort(byTime), node/cron/cron.go:64-79,220; equal times in
 * ascending rule order, one of the orders that unstable sort may give).
 * Later cg_node_result_* calls see the ordered lists; the node offsets are
 * unchanged.  Time of the pass: cg_last_kernel_times [12]. */
int cg_node_result_order_by_time(cg_ctx* ctx);
/* Order in which the per-node calls (cg_expand_per_node*, synchronous and
 * pipelined) write every node's list:
 *   CG_NODE_ORDER_RULE  rule-major (rules ascending, times ascending within a
 *                       rule) -- the default, Job.Cmds' evaluation order
 *   CG_NODE_ORDER_TIME  (time, rule): the byTime order a node's Cron keeps
 *                       (cron.go:64-79,220): the call runs the time-order
 *                       pass of cg_node_result_order_by_time itself, after
 *                       the writer (the pipelined calls enqueue it behind
 *                       each window's writer, windows of at most 4096 s; a
 *                       longer pipelined window is refused with CG_EINVAL)
 * cg_node_result_order_by_time on a result already in time order does
 * nothing. */
#define CG_NODE_ORDER_RULE 0
#define CG_NODE_ORDER_TIME 1
int cg_set_node_order(cg_ctx* ctx, int order);
/* copy the last per-node result to host buffers (node_off [N+1]; time/rule
 * [n_events], cap = their capacity); any pointer may be NULL */
int cg_node_result_copy(cg_ctx* ctx, int64_t* node_off, int64_t* time, int32_t* rule, int64_t cap);
/* copy events [first, first+count) of the last per-node result (one node's
 * list is [node_off[n], node_off[n+1])) -- what a single node's scheduler
 * fetches; either pointer may be NULL */
int cg_node_result_copy_range(cg_ctx* ctx, int64_t first, int64_t count, int64_t* time,
                              int32_t* rule);
/* Integrity check for pipelined windows (instrumentation; no reference
 * counterpart): enqueues on the ctx's stream, right behind the last enqueued
 * per-node window (or the last synchronous result), order-sensitive checksums
 * of the lists of the k nodes d_nodes[] (device int32): d_out[2i] = sum_j
 * mix(j, time[j]), d_out[2i+1] = sum_j mix(j, rule[j]) over node d_nodes[i]'s
 * list, j node-relative, mix as cg_checksum_device (device uint64 [2k]).  A
 * window past the output capacity gives zeros.  Lets a caller check windows
 * whose result a later window overwrites. */
int cg_node_checksum_enqueue(cg_ctx* ctx, const int32_t* d_nodes, int32_t k, uint64_t* d_out);
/* per-node event counts of the last per-node result, copied to a DEVICE
 * buffer of N int64 (e.g. a torch tensor for an RCCL allgather) */
int cg_node_counts_to_device(cg_ctx* ctx, int64_t* d_counts);
/* Multi-GPU per-node gather, placement step (north_star: RCCL "gathers the
 * final per-node CSR"; the node lists node/node.go:121-158 builds from
 * Job.Cmds over every job in job-ID order).  One rank's slice of the
 * per-node CSR -- d_src_node_off[N+1] (from 0), d_src_time / d_src_rule
 * (rule indices local to the rank's job-ID range) -- is copied on the ctx's
 * device so that node n's slice starts at d_dst_start[n] (= the node's global
 * offset plus the slices of the ranks before this one, from the all-gathered
 * per-node counts) in d_dst_time / d_dst_rule, rule indices plus rule_add
 * (the range's first global rule).  All pointers are device memory of the
 * ctx's device; the call returns after the copy (stream synchronised). */
int cg_node_csr_place(cg_ctx* ctx, int32_t n_nodes, const int64_t* d_src_node_off, const int64_t* d_src_time,
                      const int32_t* d_src_rule, int32_t rule_add, const int64_t* d_dst_start,
                      int64_t* d_dst_time, int32_t* d_dst_rule);
/* Multi-GPU per-node gather, merge step for TIME-ORDERED slices (the byTime
 * order every node's Cron keeps, node/cron/cron.go:64-79,220): after each
 * rank's (time, rule)-ordered slice has been placed (cg_node_csr_place), node
 * n's list in d_time / d_rule holds `world` runs in rank (= job-ID) order, run
 * g = [run_bounds[n*(world+1)+g], run_bounds[n*(world+1)+g+1]) (HOST array of
 * n_nodes*(world+1) positions, ascending).  Every node's runs are merged in
 * place into (time, rule) order -- equal times by global rule index, which
 * for job-ID-range shards is rank order -- the list one scheduler over all
 * jobs would hold.  Works through a scratch copy of node groups of at most
 * budget_bytes / 12 events (a larger node alone; never more than the events
 * being merged); world <= 64.  Returns after the merge (stream synchronised). */
int cg_node_csr_merge_ranks(cg_ctx* ctx, int32_t n_nodes, int32_t world, const int64_t* run_bounds,
                            int64_t* d_time, int32_t* d_rule, int64_t budget_bytes);

/* Device-resident rule sets: a cg_rules_in validated and copied into HBM once
 * (as specs are by cg_specs_upload), then used by any number of per-node
 * expansions on the same ctx without re-upload.  Same resolution as
 * cg_expand_per_node_device (job.go:591-630 / web/job.go:222-257). */
typedef struct cg_rules cg_rules;
int cg_rules_upload(cg_ctx* ctx, const cg_rules_in* rules, cg_rules** out);
void cg_rules_free(cg_rules* rules);
int cg_expand_per_node_rules_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z,
                                    int64_t t0, int64_t t1, const cg_rules* rules, int mode,
                                    int64_t* n_events, int64_t* nnz);
/* Pipelined per-node windows for a node scheduler's tick loop
 * (node/node.go:121-158 filtering every job, node/cron/cron.go:210-275 firing
 * them, window after window): enqueues window (t0, t1] and returns.  Window
 * k+1's rule-major expansion, rule infos, segment records and node offsets
 * run on the ctx's second stream while window k's per-node writer streams.
 * Needs an earlier cg_expand_per_node_rules_device on the same rule set and
 * exclude mode (the rule->node join, its transpose and the band width are
 * reused) whose rule-major and per-node results were at least as large as
 * every window's: a window that would exceed them writes nothing and
 * cg_expand_per_node_wait returns CG_ECAPACITY.  Every window writes the same
 * per-node output: after the wait only the LAST window's result is readable
 * (cg_node_result_*), and a returned error may belong to any window since the
 * previous wait.  The per-node result accessors refuse (CG_EINVAL) while
 * windows are pending; a synchronous call drains them and discards their
 * results and errors.  The call refuses (CG_EINVAL) while pipelined
 * rule-major calls (cg_expand_device_async) are pending: wait for them first
 * (a per-node window replaces the readable rule-major result).  cg_last_kernel_times [8] = the mean per-node writer
 * time of the waited windows. */
int cg_expand_per_node_rules_device_async(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                                          int64_t t1, const cg_rules* rules, int mode);
/* *n_events: the last window's node events (its result is then readable);
 * *n_events_all (may be NULL): the node events of every window waited for. */
int cg_expand_per_node_wait(cg_ctx* ctx, int64_t* n_events, int64_t* n_events_all);

/* ---------------------------------------------------------- fire profile --- */
/* How many commands start per bucket of time, per rule, cluster-wide and on
 * each node, over the coming day or week: the forward-looking counterpart of
 * the reference's only load view, the executed-jobs statistics kept after the
 * fact (web/info.go:14-22, job_log.go:135-150).  No fire list is written.
 *
 * Buckets are fixed-width in unix seconds: with t1 = t0 + n_buckets * width,
 * bucket b is (t0 + b*width, t0 + (b+1)*width].
 *   rule_counts[r][b]  int32, row-major [R][B]: the fires of rule r's
 *       expansion over the whole of (t0, t1] (exactly cg_expand's: @every is
 *       anchored at t0, a rule that stops stops) that fall in bucket b; a row
 *       sums to cg_count's count
 *   bucket_totals[b]   int64 [B]: the column sums
 *   node_counts[n][b]  int64, row-major [N][B]: the sum of rule_counts[r][b]
 *       over the rules node n runs under the exclude mode -- the join of
 *       cg_expand_per_node_rules_device (job.go:591-630 / web/job.go:222-257:
 *       pause, the last-rule-wins Cmd keys, all three modes), i.e. what
 *       binning the per-node lists would give
 * width < 1 or n_buckets outside [1, 4096]: CG_EINVAL; n_buckets * width >
 * CG_MAX_HORIZON: CG_ERANGE; a specs count other than the rule set's n_rules:
 * CG_EINVAL (all before any device work).  R * B may exceed 2^32 cells (10M
 * rules x 1440 buckets is 1.4e10): every index into the matrices is 64-bit,
 * and the copy accessors below take 64-bit row offsets (cg_profile_copy_rules:
 * first_rule and count are int64; the byte offset first_rule * B * 4 is formed
 * in 64 bits).  A rule whose reference loop never
 * ends inside the horizon: CG_ERANGE naming the rule, as cg_expand.  No rule:
 * valid, zero totals.
 * Synchronous, on the ctx's stream.  Like cg_count the calls drain pending
 * pipelined calls (cg_expand_device_async, the per-node windows), discard
 * their results and errors, and leave no expansion result behind.  The
 * per-node call reuses the rule->node join a per-node expansion on the same
 * rule set and mode left (and leaves its own for the next).  The profile
 * stays readable until the next profile call or cg_destroy: expansion calls
 * do not touch it.  cg_last_kernel_times [14..18]: rule matrix, walked runs,
 * totals, join + transpose (when rebuilt), node matrix. */
int cg_profile_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                      int64_t width, int32_t n_buckets);
int cg_profile_per_node_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                               int64_t width, int32_t n_buckets, const cg_rules* rules, int mode);
/* Device pointers and shape of the last profile (any out pointer may be NULL).
 * After cg_profile_device there is no node matrix: *d_node_counts = NULL,
 * *n_nodes = 0.  CG_EINVAL when no profile is readable. */
int cg_profile_result_device(cg_ctx* ctx, const int32_t** d_rule_counts,
                             const int64_t** d_bucket_totals, const int64_t** d_node_counts,
                             int64_t* n_rules, int32_t* n_nodes, int32_t* n_buckets);
/* copy rows [first, first+count) of the rule / node matrix, or the totals, to host */
int cg_profile_copy_rules(cg_ctx* ctx, int64_t first_rule, int64_t count, int32_t* out /* [count*B] */);
int cg_profile_copy_totals(cg_ctx* ctx, int64_t* out /* [B] */);
int cg_profile_copy_nodes(cg_ctx* ctx, int32_t first_node, int32_t count, int64_t* out /* [count*B] */);

/* ------------------------------------------------------ in-flight profile --- */
/* How many commands are running at each sample instant, per rule, cluster-wide
 * and on each node: starts alone do not tell whether a node can carry its
 * schedule (ten jobs that run two hours load it differently from ten that run
 * 300 ms).  The duration per rule is the caller's estimate, normally the job's
 * AvgTime (ms; job.go:62, kept up to date by Job.Avg, job.go:581-589, and
 * already the planning cost of Cmd.lockTtl, job.go:213-221).
 *
 * Buckets as above: t1 = t0 + n_buckets * width, bucket edge e_b = t0 +
 * (b+1)*width.  dur_ms[r] >= 0 is rule r's expected run time in milliseconds;
 * d_r = dur_ms[r] / 1000 rounded UP, in whole seconds.
 *   rule_counts[r][b] = #{ fires t of rule r's expansion over (t0, t1] :
 *                          e_b - d_r < t <= e_b }
 * Fire times are whole seconds, so this is exactly "started at or before e_b
 * and not yet finished at e_b" (t <= e_b < t + dur_ms/1000); that is why the
 * rounding is up.  It is not lockTtl's `cost`, which rounds AvgTime down (an
 * integer-arithmetic slip of the reference).  The expansion is cg_expand's
 * (@every anchored at t0; a rule that stops stops; a stuck rule: CG_ERANGE
 * naming it, before any cell is computed).
 * Commands started at or before t0 are unknown and NOT counted, so the first
 * d_r seconds of a row ramp up; for a warm profile start t0 earlier and drop
 * the leading buckets.
 *   bucket_totals[b]  the column sums: the cluster-wide in-flight count
 *   node_counts[n][b] the sum over the rules node n runs under the exclude
 *                     mode (the start profile's join); every node a rule is
 *                     scheduled on is counted, as the start profile counts
 *                     Cmd.Run calls
 * Not reproduced here: this profile counts every fire, also one the
 * reference would not start.  (Job.Parallels drops are the admission
 * profile's and the fires the KindAlone / KindInterval locks skip the lock
 * profile's, both below.)
 * Consequences that hold exactly: dur_ms[r] == 0 gives a zero row; d_r ==
 * width the start profile's row; d_r == m * width the sliding sum of m start
 * buckets; d_r >= n_buckets * width the prefix sums of the start row (d_r is
 * clamped to n_buckets * width, so INT64_MAX ms is valid).  A cell is at most
 * the horizon in seconds (< 2^31): the rule matrix stays int32, node matrix
 * and totals int64.
 *
 * An in-flight call is a profile call: it writes the same ctx buffers and
 * replaces the readable profile (cg_profile_result_device and
 * cg_profile_copy_* serve it unchanged), drains pending pipelined calls, shares
 * and leaves the per-node join cache, and reports its phases in
 * cg_last_kernel_times [14..18] with the same meanings.  dur_ms is a host
 * array [R] owned by the caller, copied to the device inside the call and not
 * retained.  A NULL dur_ms with R > 0, or a negative entry: CG_EINVAL naming
 * the first such rule, with the other argument checks, before any device work
 * (the previous profile stays readable). */
#define CG_PROFILE_STARTS 0
#define CG_PROFILE_INFLIGHT 1
int cg_inflight_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                       int64_t width, int32_t n_buckets, const int64_t* dur_ms /* host, [R] */);
int cg_inflight_per_node_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                                int64_t width, int32_t n_buckets, const int64_t* dur_ms /* host, [R] */,
                                const cg_rules* rules, int mode);
/* ------------------------------------------------------ admission profile --- */
/* Which fires the reference would run and which it would drop.  Cmd.Run starts
 * with Job.limit() (job.go:134-139, 165-187): when Parallels > 0 and that many
 * instances of the job are still running on the node, the fire is dropped and
 * j.Fail sends a failure notice.  KindAlone jobs are forced to Parallels = 1
 * (job.go:378-387).  A job that overruns its own period therefore runs
 * Parallels copies and fails every other fire; these calls say which, where
 * and when, ahead of time.
 *
 * Buckets, t0, w = width, B = n_buckets <= 4096, t1 = t0 + B*w, the expansion
 * over (t0, t1], @every anchored at t0 and the stuck-rule failure are the start
 * profile's.  The failure applies to a stuck rule: the call fails with
 * CG_ERANGE before any cell is computed.
 *
 * Per rule the caller gives three values:
 *   dur_ms[r] >= 0     d_r is dur_ms[r] rounded up to whole seconds and clamped
 *                      to B*w, exactly as cg_inflight_* does it
 *   parallels[r] >= 0  the value 0 means unlimited
 *   unit[r]            an int32 that does not decrease along r
 * Rules with equal unit form one unit, a contiguous rule range [u0, u1).  A
 * unit is the job's Count on one node.  All rules of a unit must carry the
 * same dur_ms and parallels; otherwise the call returns CG_EINVAL naming the
 * first rule that differs.  unit == NULL means every rule is its own unit.
 *
 * The literal process: take the fires of a unit's rules in (t0, t1] in order
 * of (time ascending, rule index ascending).  With P = parallels and d = d_r,
 * a fire at t is ADMITTED iff P == 0, or fewer than P already admitted fires a
 * of the unit have a + d > t.  Otherwise the fire is DROPPED.  Time is whole
 * seconds, so a + d > t is exactly a*1000 + dur_ms > t*1000: started and not
 * yet finished.  A fire at the very second an earlier instance ends is
 * admitted.  dur_ms == 0 admits everything.
 *   admitted[r][b] = #admitted fires of rule r in bucket b
 *   dropped[r][b]  = #dropped fires of rule r in bucket b
 *   admitted + dropped == the start profile, cell by cell
 *
 * Not reproduced:
 *   - Commands started at or before t0 are unknown.  The first d seconds
 *     therefore over-admit, which is the in-flight profile's ramp.
 *   - The reference's counter is racy for fires of the same second
 *     (job.go:170-171).  Here rule order decides.
 *   - The etcd locks of KindAlone / KindInterval across nodes are the lock
 *     profile's, below, not this one's.  An alone job is limited per node only
 *     here.
 *   - Actual run times differ from AvgTime.
 *
 * A unit with P == 0, d == 0 or P >= k*d (k its rule count: at most one fire
 * per rule per second) never drops; its rows are the start profile's.  Any
 * other unit needs P <= CG_ADMIT_MAX_PARALLELS; a larger P that can still drop
 * fails the call with CG_ERANGE naming the rule.  (The ring of admitted starts
 * shares the 64 KiB of LDS with the staged plan: a horizon whose plan exceeds
 * 46 KiB -- decades -- with a unit that can drop is CG_ERANGE too.)
 *
 * `what` is CG_PROFILE_ADMITTED, CG_PROFILE_DROPPED or CG_PROFILE_RUNNING and
 * selects the rule matrix; cg_profile_kind reports it.
 *
 * CG_PROFILE_RUNNING is the in-flight profile counting only the fires that
 * start: with the bucket edges e_b = t0 + (b+1)*w,
 *   running[r][b] = #{ admitted fires a of rule r : e_b - d_r < a <= e_b }
 * "Admitted" is the literal process above and d_r the same clamped whole
 * seconds, so a*1000 + dur_ms > e_b*1000: started and not yet finished at the
 * edge.  Rows of units that never drop are the rows of cg_inflight_device with
 * the same dur_ms.  It follows that running <= in flight cell by cell; that a
 * unit with d == w has its ADMITTED rows, one with d == m*w the sliding sum of
 * m ADMITTED buckets, one with d >= B*w their prefix sums; and that the cells
 * of a unit that can drop sum to at most P at every edge.  What is not
 * reproduced is the list below, unchanged: cold start (the rows ramp up),
 * same-second order, the locks (limit() and lock() are not composed: this kind
 * ignores the lock, CG_PROFILE_LOCK_RUNNING ignores Parallels of INTERVAL
 * jobs), Retry / Interval, actual run times.  Arguments and checks are those of
 * the other two kinds.
 *
 * The call is a profile call: it replaces
 * the readable profile, and bucket totals, the node matrix,
 * cg_profile_result_device, cg_profile_copy_*, cg_profile_node_peaks and
 * cg_profile_top_rules_* serve it as they serve the other kinds.  The node
 * matrix sums the rule rows over the rules each node runs (a rule is counted
 * on every node it is scheduled on, as before); it is exact when the rules of
 * a unit run on the same nodes, since every node then sees the same stream.
 * dur_ms, parallels and unit are host arrays [R] owned by the caller, copied
 * inside the call and not retained.  A NULL dur_ms or parallels with R > 0, a
 * negative entry, a decreasing unit, mixed dur_ms / parallels inside a unit
 * (CG_EINVAL naming the first such rule), `what` out of range (CG_EINVAL) and
 * the CG_ERANGE above are raised with the other argument checks before any
 * device work; the previous profile stays readable.
 * cg_last_kernel_times [14..18] as the start profile's, [19] the pass that
 * zeroes the rewritten rows, [20] the unit walk (k_admit_units); of a RUNNING
 * call [14], [15] are the in-flight profile's kernels and [22] the prefix sum
 * along the rewritten rows (k_rows_prefix), 0 otherwise. */
#define CG_PROFILE_ADMITTED 2
#define CG_PROFILE_DROPPED 3
#define CG_PROFILE_RUNNING 7
#define CG_ADMIT_MAX_PARALLELS 16
int cg_admit_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t width,
                    int32_t n_buckets, const int64_t* dur_ms /* host, [R] */,
                    const int64_t* parallels /* host, [R] */, const int32_t* unit /* host, [R]; may be NULL */,
                    int what);
int cg_admit_per_node_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t width,
                             int32_t n_buckets, const int64_t* dur_ms /* host, [R] */,
                             const int64_t* parallels /* host, [R] */,
                             const int32_t* unit /* host, [R]; may be NULL */, int what, const cg_rules* rules,
                             int mode);
/* ----------------------------------------------------------- lock profile --- */
/* Which fires of a KindAlone / KindInterval job run at all.  Cmd.Run, after
 * limit(), calls lock() for Kind != KindCommon (job.go:134-147): it grants a
 * lease of lockTtl() seconds and creates the key conf.Config.Lock + Job.ID only
 * if it does not exist (job.go:235-271, client.go:95-109).  The key is the
 * job's ID: one lock for all rules of the job, on all nodes.  Scheduled on m
 * nodes, such a job runs once per fire, or not at all:
 *   KindInterval  no keep-alive, and unlock() returns at once: the key lives
 *                 ttl seconds from the grant, however long the command runs
 *   KindAlone     keepAlive refreshes the lease while the command runs, and
 *                 unlock() does not revoke it but calls KeepAliveOnce: the key
 *                 lives until ttl seconds after the command ends
 * with ttl = lockTtl() computed at the fire from the rule's next two fires
 * (cg_lock_ttl_batch reproduces it).
 *
 * Buckets, t0, w = width, B = n_buckets <= 4096, t1 = t0 + B*w, the expansion
 * over (t0, t1], @every anchored at t0 and the stuck-rule failure (CG_ERANGE
 * before any cell is computed) are the start profile's.
 *
 * Inputs, all host arrays [R] owned by the caller, copied inside the call and
 * not retained:
 *   kind[r]         CG_JOB_COMMON, CG_JOB_ALONE or CG_JOB_INTERVAL
 *   avg_time_ms[r]  Job.AvgTime as stored; it may be negative (lockTtl has a
 *                   defined result for that).  d_r = ceil(max(avg, 0) / 1000),
 *                   clamped to B*w; the clamp changes nothing inside the horizon
 *   unit[r]         an int32 that does not decrease along r; NULL: every rule
 *                   is its own unit.  All rules of a unit carry the same kind
 *                   and avg_time_ms, else CG_EINVAL naming the first rule that
 *                   differs.  A unit is the job, cluster-wide: the lock key is
 *                   Job.ID, so differing node membership does not split a unit
 *                   (unlike admission)
 *   contends[r]     uint8; NULL: all ones.  0: the rule reaches no lock -- it is
 *                   scheduled on no node under the exclude mode, or replaced
 *                   everywhere by a later rule with the same Cmd key
 *   lock_ttl        conf.Config.LockTtl as in cg_lock_ttl_batch; < 2 is
 *                   CG_EINVAL (conf.go:136-138 never yields less)
 *
 * The literal process.  A lock unit is a unit with kind != COMMON.  Take the
 * fires of its contending rules in (t0, t1] in order (time ascending, rule
 * index ascending).  The state is free_at, initially -infinity.  For a fire
 * (t, r):
 *   1. If t < free_at, the fire is SKIPPED.
 *   2. Otherwise ttl = lockTtl from Next_r(t) and Next_r(Next_r(t)), kind, avg
 *      and lock_ttl: exactly what cg_lock_ttl_batch returns for now = t.  For
 *      @every D, Next_r(x) = x + D.  Both Next calls may lie past t1; they are
 *      not read off the expansion.
 *   3. If ttl == 0, the fire is skipped and the state is unchanged (lock()
 *      returns nil, job.go:246-248).
 *   4. If either Next never returns (CG_NO_PROGRESS), the call fails with
 *      CG_ERANGE naming the rule and no profile is readable afterwards.
 *   5. Otherwise the fire is GRANTED, and free_at = t + ttl for INTERVAL or
 *      t + d_r + ttl for ALONE.  (In ms the lease ends at t*1000 + max(avg, 0)
 *      + ttl*1000; for whole-second fires that is the same test.)  A fire at
 *      the very second the lease ends is granted.
 *   granted[r][b] + skipped[r][b] == the start profile, for every cell
 * Rows of COMMON units and of non-contending rules: granted is the start row,
 * skipped is zero.
 *
 * `what` is CG_PROFILE_LOCK_GRANTED, CG_PROFILE_LOCK_SKIPPED or
 * CG_PROFILE_LOCK_RUNNING and selects the rule matrix; cg_profile_kind reports
 * it.
 *
 * CG_PROFILE_LOCK_RUNNING is the in-flight profile counting only the fires that
 * are granted: with the bucket edges e_b = t0 + (b+1)*w,
 *   running[r][b] = #{ granted fires g of rule r : e_b - d_r < g <= e_b }
 * for both kinds: an INTERVAL command runs d_r seconds whatever its lease does.
 * "Granted" is the literal process above, step 4's CG_ERANGE included.  Rows of
 * COMMON units and of non-contending rules are the rows of cg_inflight_device
 * with that d_r (avg <= 0: a zero row).  running <= in flight cell by cell; a
 * unit with d == w has its GRANTED rows, d == m*w their sliding sum over m
 * buckets, d >= B*w their prefix sums; the cells of an ALONE unit sum to at
 * most 1 at every edge (free_at = g + d + ttl, ttl >= 2).  The node matrix is
 * an upper bound as GRANTED's is (which node wins a free lock is not
 * decidable); the totals count each cluster-wide run once.
 *
 * The call is a profile call: it replaces the readable profile, and bucket totals, the node matrix,
 * cg_profile_result_device, cg_profile_copy_*, cg_profile_node_peaks and
 * cg_profile_top_rules_* serve it unchanged.
 *   - The SKIPPED node row is exact: the fires of node n's Cmds at which the
 *     job ran on no node.
 *   - The GRANTED node row is an upper bound: the fires at which node n
 *     contends for a free lock.  It runs them iff it wins; which node wins is
 *     etcd arrival order, not modelled and not decidable.
 *   - The GRANTED bucket totals count each cluster-wide run once.
 *
 * Not reproduced:
 *   - Locks held at t0 are unknown (cold start).
 *   - Node clock skew.
 *   - `now` is taken as t; the reference reads the clock a little later in the
 *     same second.
 *   - Parallels of an INTERVAL job: limit() runs before lock() on each node,
 *     and whether the winner was saturated depends on who wins.  (For ALONE,
 *     limit() is subsumed: the lock is held while any instance runs.)
 *   - Job.Retry / Interval, which lengthen a run.
 *   - Actual run times differ from AvgTime.
 *   - Fires of one second are taken in rule order.
 *
 * All argument checks run before any device work, and the previous profile
 * stays readable: NULL kind or avg_time_ms with R > 0, a kind that is none of
 * the three, a decreasing unit, a mixed unit (each CG_EINVAL naming the first
 * such rule), lock_ttl < 2, `what` not 4, 5 or 8.  The zone table of the call
 * reaches from the zero time to 12 years past t1, as cg_lock_ttl_batch's; if
 * it, the plan and the walked runs' remembered positions (10 KiB) do not fit
 * the 64 KiB of LDS the call fails with CG_ERANGE.
 * cg_last_kernel_times [14..18] as the start profile's, [19] the pass that
 * zeroes the rewritten rows, [21] the unit walk (k_lock_units); [20] is 0.  Of
 * a LOCK_RUNNING call [14], [15] are the in-flight profile's kernels and [22]
 * the prefix sum along the rewritten rows (k_rows_prefix), 0 otherwise. */
#define CG_PROFILE_LOCK_GRANTED 4
#define CG_PROFILE_LOCK_SKIPPED 5
/* (6 is not assigned) */
#define CG_PROFILE_LOCK_RUNNING 8
int cg_lock_profile_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t width,
                           int32_t n_buckets, const int32_t* kind /* host, [R] */,
                           const int64_t* avg_time_ms /* host, [R] */,
                           const int32_t* unit /* host, [R]; may be NULL */,
                           const uint8_t* contends /* host, [R]; may be NULL */, int64_t lock_ttl, int what);
int cg_lock_profile_per_node_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0,
                                    int64_t width, int32_t n_buckets, const int32_t* kind /* host, [R] */,
                                    const int64_t* avg_time_ms /* host, [R] */,
                                    const int32_t* unit /* host, [R]; may be NULL */,
                                    const uint8_t* contends /* host, [R]; may be NULL */, int64_t lock_ttl,
                                    int what, const cg_rules* rules, int mode);
/* *kind = CG_PROFILE_STARTS, CG_PROFILE_INFLIGHT, CG_PROFILE_ADMITTED,
 * CG_PROFILE_DROPPED, CG_PROFILE_LOCK_GRANTED, CG_PROFILE_LOCK_SKIPPED,
 * CG_PROFILE_RUNNING or CG_PROFILE_LOCK_RUNNING: what the readable profile
 * holds.  CG_EINVAL when no profile is readable. */
int cg_profile_kind(cg_ctx* ctx, int* kind);
/* Per node row [first_node, first_node + count) of the last profile's node
 * matrix (of either kind): its largest cell and the first bucket attaining it;
 * a zero row gives (0, 0).  Computed on the device on first use after a
 * profile call and kept until the next.  CG_EINVAL when no profile is readable
 * or the last one has no node matrix. */
int cg_profile_node_peaks(cg_ctx* ctx, int32_t first_node, int32_t count, int64_t* peak /* [count] */,
                          int32_t* bucket /* [count] */);

/* ---------------------------------------------------------- fire verdicts --- */
/* Which fires those are.  The admission and lock profiles count, per bucket,
 * the fires Job.limit() drops (job.go:134-139, 165-187: a failure notice each,
 * j.Fail) and the fires the KindAlone / KindInterval lock skips (job.go:194-271:
 * a run that silently does not happen).  A verdict call marks them in the fire
 * list itself: it leaves the result of cg_expand_device(ctx, specs, z, t0, t1)
 * -- offsets[R+1], times[E], rule-major, ascending per rule, bit-identical --
 * plus verdict[E], one uint8 per fire: verdict[e] for e in [offsets[r],
 * offsets[r+1]) belongs to fire times[e] of rule r.
 *
 *   CG_VERDICT_DROPPED (bit 0)  set iff `admit` was given and the admission
 *     profile's literal process, run over (t0, t1], drops this fire
 *     (job.go:165-187): units are the maximal runs of equal unit[], a unit's
 *     fires are taken in (time, rule index) order, and a fire at t is admitted
 *     iff P == 0 or fewer than P admitted fires a of the unit have
 *     a*1000 + dur_ms > t*1000; d is dur_ms rounded up to whole seconds and
 *     clamped to t1 - t0.  Fires of units that never drop get 0.
 *   CG_VERDICT_SKIPPED (bit 1)  set iff `lock` was given and the lock profile's
 *     literal process skips this fire (job.go:235-271): t < free_at, or ttl == 0
 *     with ttl = lockTtl at now = t (job.go:194-233); a granted fire sets
 *     free_at = t + ttl (INTERVAL) or t + d + ttl (ALONE).  Fires of COMMON
 *     units and of non-contending rules get 0.
 *   Bits 2..7 are zero.  Every byte of verdict[0..E) is written by every call.
 *
 * The two bits are independent, exactly as the two profiles are: limit() and
 * lock() are not composed, and every limit the admission and lock profiles list
 * under "Not reproduced" is inherited unchanged (cold start at t0, same-second
 * order by rule index, which node wins a lock, Parallels of INTERVAL jobs,
 * Retry / Interval, actual run times, clock skew).  With t1 = t0 + B*w, binning
 * the fires with bit 0 set gives cg_admit_device(what = CG_PROFILE_DROPPED) cell
 * by cell and those without it CG_PROFILE_ADMITTED; the same holds for bit 1
 * with CG_PROFILE_LOCK_SKIPPED / CG_PROFILE_LOCK_GRANTED.
 *
 * cg_expand_verdicts_device is an expansion call: synchronous on the ctx
 * stream, it drains pending pipelined calls as cg_expand_device does and
 * replaces the readable expansion result (cg_result_device and cg_result_copy_*
 * serve it); the readable profile is untouched.  The argument structs hold host
 * arrays [R] owned by the caller, copied inside the call and not retained; their
 * members are cg_admit_device's and cg_lock_profile_device's, with the same
 * checks, messages and codes: a negative duration or parallels, a decreasing
 * unit, values that differ inside a unit, a kind that is none of the three
 * (CG_EINVAL naming the first rule), lock_ttl < 2 (CG_EINVAL), parallels above
 * CG_ADMIT_MAX_PARALLELS in a unit that can drop (CG_ERANGE).  Both structs
 * NULL, or t1 <= t0: CG_EINVAL; a horizon above CG_MAX_HORIZON: CG_ERANGE.  All
 * of these are raised before any device work and leave the previous results
 * readable.  A stuck rule (CG_ERANGE, as cg_expand_device), a granted fire
 * whose Next never returns (CG_ERANGE, as the lock profile) and a plan that
 * leaves too little LDS for the admission ring or the walked runs' positions
 * (CG_ERANGE) fail the call and leave no verdicts readable.  The walks check
 * every position against the fire list before they store; a mismatch fails the
 * call with CG_EHIP ("verdict position mismatch").  R = 0 and E = 0 are valid;
 * E may exceed 2^32.
 *
 * The accessors below return CG_EINVAL until a verdict call has succeeded, and
 * again once any later expansion call on the ctx (synchronous, pipelined,
 * per-node, count or profile) has replaced the result the bytes belong to. */
#define CG_VERDICT_DROPPED 1
#define CG_VERDICT_SKIPPED 2
/* Job.AvgTime, Job.Parallels after alone() and the admission unit per rule
 * (job.go:165-187, 378-387); host [R]; unit may be NULL */
typedef struct {
  const int64_t* dur_ms;
  const int64_t* parallels;
  const int32_t* unit;
} cg_admit_args;
/* Job.Kind, Job.AvgTime, the lock unit (the job: the key is Job.ID,
 * job.go:235-271) and whether the rule reaches the lock, per rule, and
 * conf.Config.LockTtl (job.go:194-233); host [R]; unit, contends may be NULL */
typedef struct {
  const int32_t* kind;
  const int64_t* avg_time_ms;
  const int32_t* unit;
  const uint8_t* contends;
  int64_t lock_ttl;
} cg_lock_args;
/* the expansion over (t0, t1] with its verdict bytes (job.go:134-147: limit(),
 * then lock()); admit or lock may be NULL, not both */
int cg_expand_verdicts_device(cg_ctx* ctx, const cg_specs* specs, const cg_zone* z, int64_t t0, int64_t t1,
                              const cg_admit_args* admit, const cg_lock_args* lock, int64_t* n_events);
/* the bytes in device memory, valid until the next verdict or expansion call
 * (job.go:134-147); either pointer may be NULL */
int cg_verdicts_device(cg_ctx* ctx, const uint8_t** d_verdict, int64_t* n_events);
/* verdict[first, first + count) to the host (job.go:134-147) */
int cg_verdicts_copy(cg_ctx* ctx, int64_t first, int64_t count, uint8_t* out);
/* The rule-major CSR of the fires with (verdict & mask) == value: sel_off[R+1],
 * sel_times[*n_selected], ascending per rule.  mask 1: by limit()
 * (job.go:165-187), 2: by lock() (job.go:235-271), 3: both; mask outside 1..3 or
 * value & ~mask != 0: CG_EINVAL.  The selection stays readable until the next
 * verdict, select or expansion call. */
int cg_verdicts_select_device(cg_ctx* ctx, int mask, int value, int64_t* n_selected);
/* the last selection in device memory / copied to the host (job.go:134-147);
 * CG_EINVAL when there is none */
int cg_verdicts_selected_device(cg_ctx* ctx, const int64_t** d_sel_off, const int64_t** d_sel_times,
                                int64_t* n_selected);
/* sel_off [R+1] of the last selection to the host (job.go:134-147) */
int cg_verdicts_selected_copy_offsets(cg_ctx* ctx, int64_t* out);
/* sel_times[first, first + count) of the last selection to the host (job.go:134-147) */
int cg_verdicts_selected_copy_times(cg_ctx* ctx, int64_t first, int64_t count, int64_t* out);
/* ms of the last verdict call and the last selection: the expansion (the whole
 * cg_expand_device chain with its host synchronise, plus this call's uploads of
 * the rule flags and the compacted units), the init pass, the admission walk
 * (job.go:165-187), the lock walk (job.go:235-271), the selection's count +
 * scan and its write; returns the count written (<= 6).  The first four are set
 * by a verdict call that succeeds and read 0 after one that fails; the last two
 * are set by a selection and cleared by the next verdict call. */
int cg_verdict_times(cg_ctx* ctx, float* ms, int n);

/* ---------------------------------------------- top rules of a bucket ---- */
/* Which rules make up a cell of the node matrix (or a bucket total): the peaks
 * say that a node will run 900 commands at 09:00, these calls say which rules
 * they are, without copying the rule matrix to the host.
 *
 * Take the readable profile, of either kind (CG_PROFILE_STARTS or
 * CG_PROFILE_INFLIGHT), and fix a bucket b.  A contributor of a row is a rule
 * r of that row with rule_counts[r][b] > 0.  A row's top list is its
 * contributors ordered by (count descending, rule index ascending) and cut to
 * the first k.  Per row the result holds
 *   bucket     i32     the column that was ranked
 *   n_contrib  i32     contributors of the row
 *   n_listed   i32     min(k, n_contrib)
 *   rule[k]    i32     the listed rule indices, then padding -1
 *   count[k]   i32     the listed rules' cells, then padding 0
 * Rules with a zero cell are never listed.  The sum of rule_counts[r][b] over
 * all of a node's rules is node_counts[n][b], so with k >= n_contrib the
 * listed counts sum to the node-matrix cell.  The result is deterministic:
 * the same profile gives the same bytes.
 *
 * The rows of cg_profile_top_rules_nodes are the nodes of the last per-node
 * profile, each with the rules it runs under that call's exclude mode (the
 * node-major transpose the node matrix was summed from).  That transpose is
 * the per-node path's cache, not the profile's own: a per-node call of any
 * kind with another rule set or exclude mode, or a dispatcher bind, rebuilds it
 * under the readable profile.  cg_profile_top_rules_nodes then fails with
 * CG_EINVAL ("the join the profile was built with has been replaced") rather
 * than rank against other lists; a per-node call that reuses the cached join
 * leaves it valid, and cg_profile_top_rules_bucket never depends on it.
 *
 * Errors, all raised before any device work, leaving the previous top-rules
 * result readable: k < 1 or k > CG_TOP_RULES_MAX, a bucket outside [0, B)
 * (naming the first such node), no readable profile, _nodes after a profile
 * without a node matrix or with a replaced join, pipelined calls pending:
 * CG_EINVAL.  _copy / _device without a result or with a row range outside it:
 * CG_EINVAL.  A result lives in ctx buffers of its own, readable until the
 * next top-rules call or the next profile call of either kind.  The calls
 * leave the profile, the peaks, every expansion result and
 * cg_last_kernel_times as they are. */
#define CG_TOP_RULES_MAX 64
/* every node of the last per-node profile (N rows): row n ranks bucket[n]
 * (host array [N]); bucket == NULL ranks each node's own peak bucket, i.e.
 * cg_profile_node_peaks' (computed here if not yet) -- a zero row ranks
 * bucket 0 and lists nothing */
int cg_profile_top_rules_nodes(cg_ctx* ctx, int32_t k, const int32_t* bucket);
/* cluster-wide: one row whose rules are all R rules of the profile (each rule
 * once, as bucket_totals counts them); works after cg_profile_device too */
int cg_profile_top_rules_bucket(cg_ctx* ctx, int32_t bucket, int32_t k);
/* rows [first, first+count) of the last top-rules result to the host; any
 * pointer may be NULL; rule / count are [count][k] row-major with the k of the call */
int cg_profile_top_rules_copy(cg_ctx* ctx, int32_t first, int32_t count, int32_t* rule, int32_t* cnt,
                              int32_t* n_listed, int32_t* n_contrib, int32_t* bucket);
int cg_profile_top_rules_device(cg_ctx* ctx, const int32_t** d_rule, const int32_t** d_cnt,
                                const int32_t** d_n_listed, const int32_t** d_n_contrib,
                                const int32_t** d_bucket, int32_t* rows, int32_t* k);
/* of the last top-rules call: [0] device ms of the select, [1] of the merge of
 * split rows (0 when none was split), [2] the number of chunks the rows were
 * cut into (a count, not a time); returns the entries written */
int cg_profile_top_rules_times(cg_ctx* ctx, float* ms, int n);

/* ------------------------------------------- dispatcher node fan-out ---- */
/* One dispatcher table for a whole cluster: after a wake, which node runs
 * which of the due entries.  Every cronnode runs its own Cron over its own
 * Cmds (node/node.go:121-158, node/cron/cron.go:210-275); the fan-out of a
 * wake is what those N run loops over Job.Cmds(n, groups) fire at that
 * instant: for every node n ascending, the due slots i (ascending) such that
 * rule i is scheduled on n under the exclude mode -- the set cg_rule_nodes /
 * cg_expand_per_node use (Cmd-key last-writer rule, Pause, missing groups).
 *
 *   cg_dispatcher_bind_rules  slot i of d is rule i of `rules`: builds the
 *                             rule->node CSR and its stable node-major
 *                             transpose into buffers d owns.  CG_EINVAL when
 *                             the rule set is on another ctx, the mode is
 *                             bad, d has fewer slots than the set has rules,
 *                             or pipelined per-node windows / rule-major
 *                             calls are pending on the ctx.  Binding again
 *                             rebuilds the join from scratch; an edit of single
 *                             jobs or groups is cheaper as a patch (below).
 *                             The ctx's per-node transpose cache is
 *                             dropped: the next per-node call rebuilds its own.
 *   cg_dispatcher_patch_rules  follows the watch stream (addJob / modJob /
 *                             delJob / modGroup, node/node.go:143-359) without
 *                             a rebind: rule p of `patch` is slot slot[p] of d,
 *                             and after the call that slot's node set is what
 *                             the join gives rule p inside `patch`, under the
 *                             exclude mode d was bound with.  Every slot not
 *                             named keeps its node set.  The Cmd-key
 *                             last-writer rule and the cumulative excludes act
 *                             within a job, so `patch` must hold EVERY rule of
 *                             each affected job, in the job's order, with the
 *                             node and group numbering of the bound set
 *                             (groups the patch does not reference may be left
 *                             out as missing).  slot[p] may be >= the bound
 *                             rule count, up to cg_dispatcher_count(d) - 1:
 *                             the bound rule count becomes max slot + 1 and
 *                             slots skipped in between have no nodes.  `patch`
 *                             may have more nodes than the bound set: new
 *                             nodes start with empty rows.  A rule with empty
 *                             lists, or of a paused job, gives its slot the
 *                             empty set (how a deleted job's slots are
 *                             vacated).  Afterwards the join is element for
 *                             element what cg_dispatcher_bind_rules builds
 *                             from the whole edited rule set (rule i = slot
 *                             i); the result is deterministic.  The last wake
 *                             stays valid: only its fan-out is dropped, and
 *                             cg_dispatcher_fanout may be called again for it
 *                             under the new join.  The new join is built into
 *                             spare buffers and swapped in at the end: on any
 *                             error the bound join is what it was, and a
 *                             dispatcher that has been patched holds the
 *                             join's memory twice (grow-only, released with
 *                             d).  A patch of zero rules changes nothing.
 *                             CG_EINVAL when d is unbound, `patch` is on
 *                             another ctx, a slot is < 0 or >= the
 *                             dispatcher's count, a slot appears twice, or
 *                             pipelined calls are pending (as for bind).  The
 *                             ctx's per-node transpose cache is dropped, as by
 *                             a bind.  Cost: one streaming pass over the join
 *                             (about 16 B per pair) plus a sort of the
 *                             patch's own pairs.
 *   cg_dispatcher_patch_times  ms of the last patch's device phases: [0] the
 *                             patch's join, [1] rule-major rows, [2] delta
 *                             pairs + sort, [3] removed pairs + sort, [4] merge;
 *                             returns the entries written (at most 5).
 *   cg_dispatcher_fanout      fans out the last cg_dispatcher_fire's due list;
 *                             *n_pairs = (node, slot) pairs.  The result (and
 *                             the due list) is valid until the next call on
 *                             d.  A slot >= n_rules (added by
 *                             cg_dispatcher_set past the bound set) has no
 *                             nodes until a patch names it; a replaced slot
 *                             < n_rules keeps its node set (modCmd changes
 *                             only the timer, node/node.go:219-238).
 *                             CG_EINVAL when d is
 *                             unbound or no wake was made since the last
 *                             set / remove.
 *   cg_dispatcher_fanout_copy node_off [N+1] and the slots to the host
 *                             (either may be NULL); CG_ECAPACITY naming the
 *                             required size when cap < n_pairs.
 *   cg_dispatcher_fanout_range  pairs [first, first+count) of the slots (one
 *                             node's list: first = node_off[n]).
 *   cg_dispatcher_fanout_device  the result in HBM.
 *   cg_dispatcher_set_fanout_path  instrumentation: force the dense (FILTER)
 *                             or the sparse (DUE) device path; AUTO picks.
 * cg_last_kernel_times [13] = device time of the last fan-out.
 * cg_dispatcher_fire and every other call cost what they did: the fan-out
 * runs only when asked for. */
#define CG_FANOUT_AUTO 0
#define CG_FANOUT_FILTER 1 /* stream the transpose, test each rule's due bit */
#define CG_FANOUT_DUE 2    /* expand the due slots' node lists, sort by node */
int cg_dispatcher_bind_rules(cg_dispatcher* d, const cg_rules* rules, int mode);
int cg_dispatcher_patch_rules(cg_dispatcher* d, const cg_rules* patch,
                              const int64_t* slot /* [patch n_rules] */);
int cg_dispatcher_patch_times(const cg_dispatcher* d, float* ms, int n);
int cg_dispatcher_fanout(cg_dispatcher* d, int64_t* n_pairs);
int cg_dispatcher_fanout_copy(const cg_dispatcher* d, int64_t* node_off /* [N+1] */, int32_t* slots,
                              int64_t cap);
int cg_dispatcher_fanout_range(const cg_dispatcher* d, int64_t first, int64_t count, int32_t* slots);
int cg_dispatcher_fanout_device(const cg_dispatcher* d, const int64_t** d_node_off,
                                const int32_t** d_slots, int64_t* n_pairs);
int cg_dispatcher_set_fanout_path(cg_dispatcher* d, int path);

/* ------------------------------------------- dispatcher: what fires next --- */
/* The first k entries of Cron.Entries() (node/cron/cron.go:166-174), which
 * returns the entry list in the order run() keeps it, sort.Sort(byTime):
 * earliest Next first, zero times last (cron.go:62-79,220).  Selected and
 * sorted in HBM: no snapshot of the table, no host sort.
 *
 * A FIRING entry is a slot whose Next is neither CG_ZERO_TIME nor
 * CG_NO_PROGRESS_TIME: removed slots, slots skipped by a set past the count,
 * never-firing specs and stuck slots are not firing, and byTime sorts them
 * behind every firing entry.
 *
 *   cg_dispatcher_upcoming       the first min(k, *n_total) entries of
 *                             sort.Sort(byTime) over the firing entries with
 *                             Next <= until (INT64_MAX: no bound): ascending by
 *                             Next, equal Next values in ascending slot order
 *                             (one of the orders the reference's unstable sort
 *                             may give, and the order of the due list).
 *                             *n_total = firing entries with Next <= until (so
 *                             the caller sees whether the list was cut),
 *                             *n_out = entries listed.  CG_EINVAL when k < 1
 *                             or k > CG_UPCOMING_MAX (a console page; it
 *                             covers a whole node's entry list at about 9 k
 *                             entries per node), or when pipelined calls are
 *                             pending on the ctx (as for bind_rules).  An
 *                             empty table, a table with no firing entry and an
 *                             `until` below the effective time give CG_OK and
 *                             zeros.  With until = the effective time and k >=
 *                             the count, the slots are the next
 *                             cg_dispatcher_fire's due list.
 *   cg_dispatcher_upcoming_node  the same over node `node`'s row of the bound
 *                             join (what that cronnode's own Cron.Entries()
 *                             lists first, node/node.go:121-158), under the
 *                             mode d was bound with and after any patch; slots
 *                             at or past the bound rule count are on no node.
 *                             CG_EINVAL when d is unbound or node is outside
 *                             [0, N).
 *   cg_dispatcher_upcoming_copy  the columns of the list to the host: slot
 *                             (i32), Next, Prev (i64), n_out each; any pointer
 *                             may be NULL.  CG_ECAPACITY naming the required
 *                             size when cap < n_out.
 *   cg_dispatcher_upcoming_device  the columns in HBM and n_out.
 *   cg_dispatcher_upcoming_times  of the last upcoming call: [0..2] device ms
 *                             of the select, the ordered compaction and the
 *                             sort + gather (events on the ctx stream), [3]
 *                             the streaming passes it made over the entries (a
 *                             count, not a time: at most 11, see
 *                             cg_upcoming.hip); returns the entries written
 *                             (at most 4).
 * The calls change no slot and leave the last wake, its due list and its
 * fan-out readable (buffers of their own): a peek may sit between
 * cg_dispatcher_fire and cg_dispatcher_fanout.  The list is readable until
 * the next upcoming call, or until a set / remove / fire / patch_rules /
 * bind_rules on d, which change what it describes: _copy and _device then
 * give CG_EINVAL.  The result is deterministic: the same table gives the same
 * bytes.  cg_last_kernel_times is not touched. */
#define CG_UPCOMING_MAX 65536
int cg_dispatcher_upcoming(cg_dispatcher* d, int64_t k, int64_t until,
                           int64_t* n_out, int64_t* n_total);
int cg_dispatcher_upcoming_node(cg_dispatcher* d, int32_t node, int64_t k, int64_t until,
                                int64_t* n_out, int64_t* n_total);
int cg_dispatcher_upcoming_copy(const cg_dispatcher* d, int32_t* slots, int64_t* next,
                                int64_t* prev, int64_t cap);
int cg_dispatcher_upcoming_device(const cg_dispatcher* d, const int32_t** d_slots,
                                  const int64_t** d_next, const int64_t** d_prev, int64_t* n);
int cg_dispatcher_upcoming_times(const cg_dispatcher* d, float* ms, int n);

/* ------------------------------------------- multi-GPU (RCCL over xGMI) --- */
/* One process (or thread) per MI355X, each with its own cg_ctx; rules shard
 * by contiguous job-ID ranges with no data-path collective (every cronsun
 * node filters every job itself, node/node.go:121-141; here a rank evaluates
 * one range of jobs for every node).  The only exchanges (north_star) are the
 * all-gather of per-node event counts / offsets and the gather of the final
 * per-node CSR.  RCCL is loaded at run time (see below); CG_ENODEV if absent.
 *
 *   cg_comm_unique_id   ncclGetUniqueId: rank 0 makes the id, the caller
 *                       hands it to every rank (any channel)
 *   cg_comm_init        ncclCommInitRank on the ctx's device (collective)
 *   cg_comm_allgather_i64  all[g*n + i] = rank g's mine[i] (host buffers;
 *                       event totals -> global rule-major offsets, per-block
 *                       weights of the event-balanced cut)
 *   cg_comm_node_offsets   all-gather of the per-node event counts of every
 *                       rank's last per-node result (N int64 per rank):
 *                       node_start[n] = node_base[n] + the counts of the
 *                       ranks before this one (where this rank's slice of
 *                       node n lands in the job-ID-ordered global list),
 *                       node_base[N+1] the global node offsets (host; either
 *                       may be NULL)
 *   cg_comm_gather_node_csr  every rank's last per-node result gathered on
 *                       `root` into the caller's DEVICE buffers
 *                       d_node_off [N+1], d_time / d_rule [cap] (root only;
 *                       ignored elsewhere): node n's global list is the ranks'
 *                       slices in rank (= job-ID) order, rule indices made
 *                       global by each rank's rule_base (its range's first
 *                       global rule).  When every rank's result is in (time,
 *                       rule) order (CG_NODE_ORDER_TIME), root merges each
 *                       node's slices into one (time, rule)-ordered list
 *                       (cg_node_csr_merge_ranks), the byTime list of one
 *                       scheduler over every job; ranks mixing the two orders
 *                       are refused, and so are time-ordered results of more
 *                       than 64 ranks or whose rule_base does not ascend with
 *                       the rank among the ranks holding events (the merge
 *                       breaks time ties by rank), on every rank before any
 *                       transfer.  The payload moves in chunks of whole
 *                       node ranges (a node larger than the budget in parts)
 *                       whose peer bytes (12 B per event) stay within
 *                       budget_bytes (the smallest any rank passes; at least
 *                       24 B per rank), so root's staging is bounded by it;
 *                       grouped ncclSend/ncclRecv per chunk, placed on root by
 *                       a kernel (root's staging, also the merge's scratch:
 *                       at most the budget, or the largest node when a time-
 *                       ordered node exceeds it).  Every rank returns the same
 *                       status: CG_ECAPACITY when the total exceeds root's
 *                       cap, CG_EINVAL when a rank has no readable result, the
 *                       node counts or list orders differ, and root's
 *                       allocation failure on every rank.  A transfer that
 *                       fails after all ranks agreed aborts the communicator
 *                       (later calls fail with CG_EHIP).  *n_events = the
 *                       global total.
 *   cg_comm_gather_plan the gather's chunk plan, host only (no device, no
 *                       communicator): counts [world * n_nodes] per-node event
 *                       counts of every rank; chunks[4i..4i+3] = {n0, n1, j,
 *                       k}: nodes [n0, n1) whole (k == 1), or part j of k of
 *                       node n0, rank g's part being its events [c*j/k,
 *                       c*(j+1)/k) of that node.  *n_chunks always set;
 *                       CG_ECAPACITY when it exceeds cap.
 * Collective calls must be made by every rank of the comm, in the same order.
 * RCCL is loaded by full path with local symbol scope, one copy per process:
 * one already mapped, else the librccl.so beside the HIP runtime the library
 * runs on, else /opt/rocm/lib; when a different RCCL is mapped later the
 * cg_comm calls fail with CG_EINVAL naming both. */
typedef struct cg_comm cg_comm;
#define CG_COMM_ID_BYTES 128
int cg_comm_unique_id(uint8_t id[CG_COMM_ID_BYTES]);
int cg_comm_init(cg_ctx* ctx, int world, int rank, const uint8_t id[CG_COMM_ID_BYTES], cg_comm** out);
void cg_comm_free(cg_comm* comm);
int cg_comm_allgather_i64(cg_comm* comm, const int64_t* mine, size_t n, int64_t* all);
int cg_comm_node_offsets(cg_comm* comm, int64_t* node_start, int64_t* node_base);
int cg_comm_gather_node_csr(cg_comm* comm, int root, int64_t rule_base, int64_t budget_bytes,
                            int64_t* d_node_off, int64_t* d_time, int32_t* d_rule, int64_t cap,
                            int64_t* n_events);
int cg_comm_gather_plan(const int64_t* counts, int32_t world, int32_t n_nodes, int32_t root,
                        int64_t budget_bytes, int64_t* chunks, int64_t cap, int64_t* n_chunks);

/* rule -> node CSR only (GPU join), host output */
int cg_rule_nodes(cg_ctx* ctx, const cg_rules_in* rules, int mode, int64_t* rn_off /*[R+1]*/,
                  int32_t* rn_nodes, int64_t cap, int64_t* nnz);

/* ----------------------------------- string-keyed job model (host) --- */
/* Host interning of cronsun's string IDs (Job/JobRule/Group, job.go:38-84,
 * group.go:17-22) into cg_rules_in.  Job IDs, rule IDs, group IDs and node
 * IDs are arbitrary byte strings (NUL-terminated here). */
int cg_jobset_new(cg_jobset** out);
void cg_jobset_free(cg_jobset* js);
int cg_jobset_add_group(cg_jobset* js, const char* gid, const char* const* nids, size_t n);
int cg_jobset_add_job(cg_jobset* js, const char* job_id, int pause);
/* appends a rule to the last added job */
int cg_jobset_add_rule(cg_jobset* js, const char* rule_id, const char* const* gids, size_t ng,
                       const char* const* nids, size_t nn, const char* const* ex, size_t ne);
/* freeze and expose the interned arrays (valid until the jobset is freed) */
int cg_jobset_rules(cg_jobset* js, cg_rules_in* out);
/* node index of a node ID (-1 if unknown) / node ID of an index */
int32_t cg_jobset_node_index(const cg_jobset* js, const char* nid);
const char* cg_jobset_node_id(const cg_jobset* js, int32_t idx);
/* Job.Cmds(nid, groups) keys (job.go:591-614): writes the rule indices of
 * the job's Cmds on node nid -- after the map's last-writer-wins dedup of
 * Job.ID+Rule.ID -- and returns their count (host reference semantics). */
int32_t cg_jobset_cmds(const cg_jobset* js, int32_t job, const char* nid, int32_t* rules_out,
                       int32_t cap);
/* Job.IsRunOn(nid, groups) (job.go:616-630) */
int cg_jobset_is_run_on(const cg_jobset* js, int32_t job, const char* nid);
/* Job.GetJobNodes (web/job.go:222-257): node indices in first-seen order */
int32_t cg_jobset_job_nodes(const cg_jobset* js, int32_t job, int32_t* nodes_out, int32_t cap);

/* ------------------------------------------ bulk ingestion (etcd JSON) --- */
/* GetGroups("") / GetJobs() (group.go:39-63, job.go:339-365) over the raw
 * etcd values: docs[i] is the JSON value of one key under /cronsun/group/
 * (groups) or /cronsun/cmd/ (jobs), in key order.  Each value goes through
 * json.Unmarshal into Group / Job (Go 1.7-1.8 encoding/json semantics, see
 * cg_ingest.cpp), Job.Valid (every rule's Timer through cron.Parse) and
 * alone(); the last valid value of an ID wins.  Decoding runs on nthreads
 * host threads.  status[i] (optional) gets one of: */
#define CG_INGEST_OK 0          /* added to the jobset */
#define CG_INGEST_UNMARSHAL 1   /* json.Unmarshal error: skipped (job.go:353-356) */
#define CG_INGEST_INVALID 2     /* Job.Valid error (ErrNilRule, parse error): skipped */
#define CG_INGEST_PANIC 3       /* a null rule: the reference panics in JobRule.Valid */
#define CG_INGEST_REPLACED 4    /* a later value with the same ID replaced it */
#define CG_INGEST_UNSUPPORTED 5 /* an ID containing NUL (not representable here) */
int cg_jobset_ingest_groups(cg_jobset* js, const char* const* docs, const size_t* lens, size_t n,
                            int nthreads, int32_t* status);
int cg_jobset_ingest_jobs(cg_jobset* js, const char* const* docs, const size_t* lens, size_t n,
                          int nthreads, int32_t* status);
/* JobRule.Schedule per rule (rule order of cg_jobset_rules); returns the rule
 * count (writes at most cap).  CG_EINVAL if a rule was added without a timer. */
int cg_jobset_schedules(const cg_jobset* js, cg_schedule* out, size_t cap);
/* Job.Kind, Job.AvgTime (ms) and Job.Parallels (after alone()) per job;
 * returns the job count (writes at most cap; any pointer may be NULL) */
int cg_jobset_job_meta(const cg_jobset* js, int32_t* kind, int64_t* avg_time_ms,
                       int64_t* parallels, size_t cap);
const char* cg_jobset_job_id(const cg_jobset* js, int32_t job);
const char* cg_jobset_group_id(const cg_jobset* js, int32_t group);
const char* cg_jobset_rule_id(const cg_jobset* js, int32_t rule);

#ifdef __cplusplus
}
#endif
#endif /* CRONSUN_GPU_H */
