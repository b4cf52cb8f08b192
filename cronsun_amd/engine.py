"""Batch engine over one MI355X: the node/cron/gpu package of the design,
seen from Python.  Wraps a cg_ctx (one HIP device + stream + HBM buffers).

  Engine.upload(schedules)                  -> Specs (SoA packed in HBM)
  Engine.next_batch(specs, loc, t)          Schedule.Next for every rule
  Engine.lock_ttl_batch(specs, loc, now, kind, avg_time_ms, lock_ttl)
                                            Cmd.lockTtl for every rule
  Engine.dispatcher(specs, loc, now)        Cron.run's entry state in HBM
  Engine.expand(specs, loc, t0, t1)         rule-major CSR of fire times
  Engine.expand_device(specs, loc, t0, t1)  same, left in HBM (bench)
  Engine.expand_per_node(specs, loc, t0, t1, rules, mode)
                                            per-node (time, rule) CSR
  Engine.profile(specs, loc, t0, width, n_buckets)
                                            fires per (rule, bucket), no lists
  Engine.profile_per_node(specs, loc, t0, width, n_buckets, drules, mode)
                                            fires per (node, bucket)
  Engine.inflight(specs, loc, t0, width, n_buckets, dur_ms)
                                            commands running per (rule, bucket edge)
  Engine.inflight_per_node(specs, loc, t0, width, n_buckets, dur_ms, drules, mode)
                                            ... per (node, bucket edge)
  Engine.admit(specs, loc, t0, width, n_buckets, dur_ms, parallels, unit, what)
                                            fires Job.limit() admits / drops per (rule, bucket)
  Engine.admit_per_node(specs, loc, t0, width, n_buckets, dur_ms, parallels, unit, drules, mode, what)
                                            ... per (node, bucket)
  Engine.lock_runs(specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit, contends, lock_ttl, what)
                                            fires the KindAlone / KindInterval lock grants / skips
  Engine.lock_runs_per_node(specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit, contends, drules, mode, lock_ttl, what)
                                            ... per (node, bucket)
  Engine.expand_verdicts(specs, loc, t0, t1, admit, lock)
                                            expand() plus one byte per fire: dropped / lock-skipped
  Engine.verdicts_select(mask, value)       rule-major CSR of the fires with those bits
  Engine.profile_node_peaks()               per node: largest cell, first bucket with it
  Engine.profile_top_rules(k, buckets=None) per node: the k rules with the largest
                                            cells of one bucket (default: its peak)
  Engine.profile_top_rules_bucket(bucket, k)
                                            the same over all rules, cluster-wide
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import CgError, check, lib


class Specs:
    """An uploaded rule set (device-resident, 32 B per rule)."""

    def __init__(self, engine, handle, n, parent=None):
        self.engine = engine
        self._h = handle
        self.n = n
        self._parent = parent  # keeps the parent of a slice alive

    def __len__(self):
        return self.n

    def slice(self, first, count):
        h = C.c_void_p()
        check(lib().cg_specs_slice(self._h, first, count, C.byref(h)))
        return Specs(self.engine, h, count, parent=self)

    def free(self):
        if self._h:
            lib().cg_specs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceRules:
    """An uploaded rule set (cg_rules): the interned jobs/groups in HBM."""

    def __init__(self, engine, handle, rules):
        self.engine = engine
        self._h = handle
        self.n_rules, self.n_nodes = rules.n_rules, rules.n_nodes

    def free(self):
        if self._h:
            lib().cg_rules_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """The library's RCCL communicator (cg_comm_*): one rank per MI355X, bound
    to an Engine's device and stream.  unique_id() on rank 0, handed to every
    rank (e.g. torch.distributed.broadcast_object_list), then Comm(engine,
    world, rank, id) on every rank."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(lib().cg_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, engine, world, rank, uid):
        if len(uid) != 128:
            raise ValueError("RCCL unique id must be 128 bytes")
        self.engine, self.world, self.rank = engine, int(world), int(rank)
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        check(lib().cg_comm_init(engine._h, self.world, self.rank, buf, C.byref(h)))
        self._h = h

    def allgather_i64(self, values):
        """all[g, i] = rank g's values[i] (host int64)."""
        mine = np.ascontiguousarray(values, dtype=np.int64)
        out = np.zeros((self.world, mine.size), dtype=np.int64)
        check(lib().cg_comm_allgather_i64(self._h, mine.ctypes.data, mine.size, out.ctypes.data))
        return out

    def node_offsets(self, n_nodes):
        """(node_start [N], node_base [N+1]) of every rank's last per-node result
        (the all-gather of per-node counts)."""
        start = np.zeros(max(n_nodes, 1), dtype=np.int64)
        base = np.zeros(n_nodes + 1, dtype=np.int64)
        check(lib().cg_comm_node_offsets(self._h, start.ctypes.data, base.ctypes.data))
        return start[:n_nodes], base

    def gather_node_csr(self, root, rule_base, budget_bytes, d_node_off=0, d_time=0, d_rule=0, cap=0):
        """cg_comm_gather_node_csr into device pointers (root); returns the
        global node-event total."""
        n = C.c_int64()
        check(lib().cg_comm_gather_node_csr(self._h, int(root), int(rule_base), int(budget_bytes),
                                            d_node_off or None, d_time or None, d_rule or None, int(cap),
                                            C.byref(n)))
        return n.value

    def free(self):
        if getattr(self, "_h", None):
            lib().cg_comm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Dispatcher:
    """Cron.run's entries (node/cron/cron.go:210-275) resident in HBM
    (cg_dispatcher_*): slots with a schedule, Next and Prev."""

    def __init__(self, engine, handle):
        self.engine = engine
        self._h = handle

    def __len__(self):
        return int(lib().cg_dispatcher_count(self._h))

    @property
    def effective(self):
        """The earliest non-zero Next (ZERO_TIME: nothing can fire)."""
        e = C.c_int64()
        check(lib().cg_dispatcher_effective(self._h, C.byref(e)))
        return e.value

    def fire(self, now):
        """One wake at `now` >= effective: the due slots (ascending) and the
        next effective time."""
        n, e = C.c_int64(), C.c_int64()
        check(lib().cg_dispatcher_fire(self._h, int(now), C.byref(n), C.byref(e)))
        due = np.empty(max(n.value, 1), dtype=np.int32)
        check(lib().cg_dispatcher_due(self._h, 0, n.value, due.ctypes.data))
        return due[:n.value], e.value

    def fire_count(self, now):
        """One wake, leaving the due list in HBM: (n_due, next effective)."""
        n, e = C.c_int64(), C.c_int64()
        check(lib().cg_dispatcher_fire(self._h, int(now), C.byref(n), C.byref(e)))
        return n.value, e.value

    def set(self, idx, schedules, now):
        """Add or replace entries: slot idx[j] <- schedules[j], Next = Next(now)."""
        ix = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        arr = _as_c_schedules(schedules)
        check(lib().cg_dispatcher_set(self._h, ix.ctypes.data, C.cast(arr, C.c_void_p), len(ix),
                                      int(now)))

    def remove(self, idx):
        ix = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        check(lib().cg_dispatcher_remove(self._h, ix.ctypes.data, len(ix)))

    # ------------------------------------------------------ node fan-out
    def bind_rules(self, drules, mode=_lib.EXCLUDE_NONE):
        """Slot i is rule i of the uploaded rule set `drules`: builds the
        rule -> node join the fan-out of a wake uses (an edit of single jobs
        or groups: patch_rules)."""
        check(lib().cg_dispatcher_bind_rules(self._h, drules._h, int(mode)))
        self._n_nodes = drules.n_nodes

    def patch_rules(self, drules, slots):
        """Rule p of the uploaded patch `drules` is slot slots[p]: that slot's
        node set becomes what the join gives rule p inside the patch (under
        the mode of bind_rules); every other slot keeps its own.  The patch
        holds every rule of each affected job, in the job's order, with the
        bound set's node and group numbering; slots may lie past the bound
        rule count (after set) and the patch may bring new nodes.  The last
        wake stays valid: fanout() gives it again under the new join."""
        sl = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int64)
        if sl.shape != (drules.n_rules,):
            raise ValueError("patch_rules: one slot per patch rule")
        check(lib().cg_dispatcher_patch_rules(self._h, drules._h, sl.ctypes.data))
        if drules.n_rules:
            self._n_nodes = max(getattr(self, "_n_nodes", 0), drules.n_nodes)

    def patch_ms(self):
        """Device ms of the last patch_rules by phase: the patch's join,
        rule-major rows, delta pairs + sort, removed pairs + sort, merge."""
        buf = (C.c_float * 5)()
        n = check(lib().cg_dispatcher_patch_times(self._h, buf, 5))
        return list(buf)[:n]

    def set_fanout_path(self, path):
        """CG_FANOUT_AUTO (default) / _FILTER / _DUE: force a device path
        (instrumentation)."""
        check(lib().cg_dispatcher_set_fanout_path(self._h, int(path)))

    def fanout_count(self):
        """Fan the last wake out to nodes, leaving the result in HBM: the
        number of (node, slot) pairs."""
        n = C.c_int64()
        check(lib().cg_dispatcher_fanout(self._h, C.byref(n)))
        return n.value

    def fanout(self):
        """The last wake fanned out to nodes: (node_off [N+1], slots) -- node
        n runs slots[node_off[n]:node_off[n+1]], ascending."""
        n = self.fanout_count()
        node_off = np.empty(getattr(self, "_n_nodes", 0) + 1, dtype=np.int64)
        slots = np.empty(max(n, 1), dtype=np.int32)
        check(lib().cg_dispatcher_fanout_copy(self._h, node_off.ctypes.data, slots.ctypes.data, n))
        return node_off, slots[:n]

    def fanout_range(self, first, count):
        """Pairs [first, first+count) of the last fan-out's slots (one node's
        list: first = node_off[n])."""
        out = np.empty(max(int(count), 1), dtype=np.int32)
        check(lib().cg_dispatcher_fanout_range(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def fanout_device(self):
        """(node_off pointer, slots pointer, n_pairs) of the last fan-out in HBM."""
        off, sl, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().cg_dispatcher_fanout_device(self._h, C.byref(off), C.byref(sl), C.byref(n)))
        return off.value, sl.value, n.value

    # ---------------------------------------------------- what fires next
    def upcoming_count(self, k, until=None, node=None):
        """Select the first k entries of Cron.Entries() (byTime order: Next
        ascending, equal Next by slot) among the firing entries with
        Next <= until, cluster-wide or over node `node`'s row of the bound
        join, leaving the list in HBM: (n_out, n_total) -- entries listed,
        firing entries with Next <= until."""
        n, tot = C.c_int64(), C.c_int64()
        u = (1 << 63) - 1 if until is None else int(until)
        if node is None:
            check(lib().cg_dispatcher_upcoming(self._h, int(k), u, C.byref(n), C.byref(tot)))
        else:
            check(lib().cg_dispatcher_upcoming_node(self._h, int(node), int(k), u, C.byref(n), C.byref(tot)))
        self.upcoming_total = tot.value
        return n.value, tot.value

    def upcoming_copy(self, n):
        """(slots, next, prev) of the last upcoming list, n entries each."""
        m = max(int(n), 1)
        sl, nx, pv = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int64), np.empty(m, dtype=np.int64)
        check(lib().cg_dispatcher_upcoming_copy(self._h, sl.ctypes.data, nx.ctypes.data, pv.ctypes.data, int(n)))
        return sl[:n], nx[:n], pv[:n]

    def upcoming(self, k, until=None, node=None):
        """The next k entries to fire: (slots, next, prev), byTime order.  The
        number of firing entries with Next <= until is left in
        self.upcoming_total (larger than len(slots): the list was cut)."""
        n, _ = self.upcoming_count(k, until, node)
        return self.upcoming_copy(n)

    def upcoming_device(self):
        """(slots pointer, next pointer, prev pointer, n) of the last upcoming
        list in HBM."""
        sl, nx, pv, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().cg_dispatcher_upcoming_device(self._h, C.byref(sl), C.byref(nx), C.byref(pv), C.byref(n)))
        return sl.value, nx.value, pv.value, n.value

    def upcoming_ms(self):
        """Of the last upcoming call: device ms of [select, compaction, sort +
        gather], and the streaming passes it made over the entries."""
        buf = (C.c_float * 4)()
        n = check(lib().cg_dispatcher_upcoming_times(self._h, buf, 4))
        v = list(buf)[:n]
        return v[:3], int(v[3])

    def snapshot(self):
        """(next, prev, live) per slot."""
        n = len(self)
        nx = np.empty(max(n, 1), dtype=np.int64)
        pv = np.empty(max(n, 1), dtype=np.int64)
        lv = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().cg_dispatcher_snapshot(self._h, nx.ctypes.data, pv.ctypes.data, lv.ctypes.data))
        return nx[:n], pv[:n], lv[:n].astype(bool)

    def free(self):
        if self._h:
            lib().cg_dispatcher_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_c_schedules(schedules):
    if isinstance(schedules, C.Array) and schedules._type_ is _lib.cg_schedule:
        return schedules  # already a cg_schedule array (cron.parse_batch, a numpy view)
    arr =(_lib.cg_schedule * max(len(schedules), 1))()
    for i, s in enumerate(schedules):
        arr[i] = s.to_c() if hasattr(s, "to_c") else s
    return arr


class RulesIn:
    """Integer-interned jobs/groups (cg_rules_in).  Arrays are numpy and kept
    alive by this object."""

    FIELDS = ("group_off", "group_nodes", "group_exists", "rule_job", "nid_off", "nids",
              "gid_off", "gids", "ex_off", "ex", "job_pause")
    DTYPES = {"group_off": np.int64, "group_nodes": np.int32, "group_exists": np.uint8,
              "rule_job": np.int32, "nid_off": np.int64, "nids": np.int32, "gid_off": np.int64,
              "gids": np.int32, "ex_off": np.int64, "ex": np.int32, "job_pause": np.uint8}

    def __init__(self, n_nodes, n_groups, n_rules, n_jobs, rule_key=None, **arrays):
        """rule_key (optional, [R]): the rules' Cmd keys (Job.ID+Rule.ID,
        job.go:130-132) interned so that two rules of one job compare equal
        exactly when their Rule.IDs are; None = every rule its own key."""
        self.n_nodes, self.n_groups, self.n_rules, self.n_jobs = n_nodes, n_groups, n_rules, n_jobs
        for f in self.FIELDS:
            a = np.ascontiguousarray(arrays[f], dtype=self.DTYPES[f])
            if a.size == 0:
                a = np.zeros(1, dtype=self.DTYPES[f])
            setattr(self, f, a)
        self.rule_key = None
        if rule_key is not None:
            k = np.ascontiguousarray(rule_key, dtype=np.int32)
            if k.shape != (n_rules,):
                raise ValueError("rule_key must hold one key per rule")
            self.rule_key = k if k.size else np.zeros(1, dtype=np.int32)

    def slice_rules(self, lo, hi):
        """The rules [lo, hi) as their own rule set (job-ID-range shard): the
        same nodes and groups, the jobs of those rules renumbered from 0.  A
        job's rules must not be split by the cut."""
        if lo < 0 or hi > self.n_rules or lo > hi:
            raise ValueError("rule range out of bounds")
        if 0 < lo < self.n_rules and self.rule_job[lo - 1] == self.rule_job[lo]:
            raise ValueError("the cut splits a job's rules")
        if 0 < hi < self.n_rules and self.rule_job[hi - 1] == self.rule_job[hi]:
            raise ValueError("the cut splits a job's rules")
        rj = self.rule_job[lo:hi]
        j0 = int(rj[0]) if hi > lo else 0
        j1 = int(rj[-1]) + 1 if hi > lo else 0

        def part(off, vals):
            o = off[lo:hi + 1] - off[lo]
            return o, vals[off[lo]:off[hi]]
        nid_off, nids = part(self.nid_off, self.nids)
        gid_off, gids = part(self.gid_off, self.gids)
        ex_off, ex = part(self.ex_off, self.ex)
        return RulesIn(self.n_nodes, self.n_groups, hi - lo, j1 - j0,
                       group_off=self.group_off, group_nodes=self.group_nodes,
                       group_exists=self.group_exists, rule_job=rj - j0, nid_off=nid_off, nids=nids,
                       gid_off=gid_off, gids=gids, ex_off=ex_off, ex=ex,
                       job_pause=self.job_pause[j0:j1],
                       rule_key=None if self.rule_key is None else self.rule_key[lo:hi])

    def to_c(self):
        s = _lib.cg_rules_in()
        s.n_nodes, s.n_groups, s.n_rules, s.n_jobs = (
            self.n_nodes, self.n_groups, self.n_rules, self.n_jobs)
        for f in self.FIELDS:
            setattr(s, f, getattr(self, f).ctypes.data)
        s.rule_key = self.rule_key.ctypes.data if self.rule_key is not None else None
        return s


class Engine:
    def __init__(self, device=0):
        self._lock = threading.Lock()
        h = C.c_void_p()
        check(lib().cg_init(device, C.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().cg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ specs
    def upload(self, schedules):
        arr = _as_c_schedules(schedules)
        h = C.c_void_p()
        check(lib().cg_specs_upload_schedules(self._h, C.cast(arr, C.c_void_p), len(schedules),
                                              C.byref(h)))
        return Specs(self, h, len(schedules))

    def upload_c(self, arr, n):
        """Upload a ctypes array of cg_schedule (e.g. from cron.parse_batch)."""
        h = C.c_void_p()
        check(lib().cg_specs_upload_schedules(self._h, C.cast(arr, C.c_void_p), n, C.byref(h)))
        return Specs(self, h, n)

    def upload_soa(self, second, minute, hour, dom, month, dow, delay_ns):
        """SoA upload (cg_specs_upload): delay_ns[i] > 0 makes rule i an @every
        of that delay, else its six masks are read.  A mask column may be None
        (NULL: reads as zero)."""
        d = np.ascontiguousarray(delay_ns, dtype=np.int64)
        cols = [None if x is None else np.ascontiguousarray(x, dtype=np.uint64)
                for x in (second, minute, hour, dom, month, dow)]
        if any(c is not None and c.shape != d.shape for c in cols):
            raise ValueError("upload_soa: one mask per rule in every column")
        soa = _lib.cg_spec_soa(*[None if c is None else c.ctypes.data for c in cols], d.ctypes.data)
        h = C.c_void_p()
        check(lib().cg_specs_upload(self._h, C.byref(soa), len(d), C.byref(h)))
        return Specs(self, h, len(d))

    def _specs(self, specs):
        return specs if isinstance(specs, Specs) else self.upload(specs)

    @staticmethod
    def _loc(loc):
        if loc is None:
            from .cron import UTC
            return UTC()
        return loc

    # ------------------------------------------------------------- Next
    def next_batch(self, specs, loc, t_in):
        sp = self._specs(specs)
        t = np.ascontiguousarray(t_in, dtype=np.int64)
        if t.shape[0] != sp.n:
            raise ValueError("one input time per rule")
        out = np.empty_like(t)
        check(lib().cg_next_batch(self._h, sp._h, self._loc(loc).handle, t.ctypes.data,
                                  out.ctypes.data))
        return out

    def lock_ttl_batch(self, specs, loc, now, kind, avg_time_ms, lock_ttl=300):
        """Cmd.lockTtl (job.go:194-233) per rule at time now[i] (scalar or
        per rule): the lease TTL in seconds, 0 for a rule that never fires.
        kind = Job.Kind, avg_time_ms = Job.AvgTime, lock_ttl = conf LockTtl."""
        sp = self._specs(specs)
        n = sp.n
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(now, dtype=np.int64), (n,)))
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(kind, dtype=np.int32), (n,)))
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(avg_time_ms, dtype=np.int64), (n,)))
        out = np.empty(n, dtype=np.int64)
        check(lib().cg_lock_ttl_batch(self._h, sp._h, self._loc(loc).handle, t.ctypes.data,
                                      k.ctypes.data, a.ctypes.data, int(lock_ttl),
                                      out.ctypes.data))
        return out

    def dispatcher(self, specs, loc, now):
        """Cron.run start (cron.go:212-215) over `specs` at `now`."""
        sp = self._specs(specs)
        h = C.c_void_p()
        rc = lib().cg_dispatcher_new(self._h, sp._h, self._loc(loc).handle, int(now), C.byref(h))
        if rc < 0 and h:
            # a stuck entry (CG_ERANGE): the dispatcher was built and handed
            # back with the error; keep the message, free the table
            err = CgError(rc, _lib.last_error())
            lib().cg_dispatcher_free(h)
            raise err
        check(rc)
        return Dispatcher(self, h)

    # -------------------------------------------------------- expansion
    def expand(self, specs, loc, t0, t1):
        sp = self._specs(specs)
        n = C.c_int64()
        check(lib().cg_expand_device(self._h, sp._h, self._loc(loc).handle, int(t0), int(t1),
                                     C.byref(n)))
        off = np.empty(sp.n + 1, dtype=np.int64)
        check(lib().cg_result_copy_offsets(self._h, off.ctypes.data))
        times = np.empty(max(n.value, 1), dtype=np.int64)
        check(lib().cg_result_copy_times(self._h, 0, n.value, times.ctypes.data))
        return off, times[:n.value]

    def count(self, specs, loc, t0, t1):
        """Fires per rule in (t0, t1] (count pass only, cg_count)."""
        sp = self._specs(specs)
        out = np.empty(max(sp.n, 1), dtype=np.int64)
        tot = C.c_int64()
        check(lib().cg_count(self._h, sp._h, self._loc(loc).handle, int(t0), int(t1),
                             out.ctypes.data, C.byref(tot)))
        return out[:sp.n]

    def expand_device(self, specs, loc, t0, t1):
        n = C.c_int64()
        check(lib().cg_expand_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(t1),
                                     C.byref(n)))
        return n.value

    def expand_async(self, specs, loc, t0, t1):
        """Enqueue a pipelined expansion (cg_expand_device_async): returns at
        once; results and errors come with expand_wait()."""
        check(lib().cg_expand_device_async(self._h, specs._h, self._loc(loc).handle, int(t0), int(t1)))

    def expand_wait(self):
        """Wait for the async expansions since the last wait; the event total of
        the last one (its result is then the engine's current result)."""
        n = C.c_int64()
        check(lib().cg_expand_wait(self._h, C.byref(n)))
        return n.value

    def set_async_overlap(self, on):
        """Pipelined expansions alternate between two writer streams and output
        buffers (default, when the second buffer fits) or use one
        (cg_set_async_overlap); refused while calls are pending."""
        check(lib().cg_set_async_overlap(self._h, 1 if on else 0))

    def result_device(self):
        off, times, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().cg_result_device(self._h, C.byref(off), C.byref(times), C.byref(n)))
        return off.value, times.value, n.value

    def copy_times(self, first, count):
        out = np.empty(max(count, 1), dtype=np.int64)
        check(lib().cg_result_copy_times(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def kernel_times(self):
        """ms per phase of the last expansion: count, scan, block map,
        write(closed form), write(walk), offsets."""
        buf = (C.c_float * 12)()
        k = lib().cg_last_kernel_times(self._h, buf, 12)
        return list(buf)[:min(k, 6)]

    def set_phase_timing(self, level):
        """2: HIP events between all expansion phases (default); 1: around
        k_write_cf only (the other phases then read -1)."""
        check(lib().cg_set_phase_timing(self._h, int(level)))

    def node_kernel_times(self):
        """ms per phase of the last per-node call: rule->node join,
        transpose + per-node offsets, per-node write."""
        buf = (C.c_float * 12)()
        lib().cg_last_kernel_times(self._h, buf, 12)
        return list(buf)[6:9]

    def dispatch_kernel_times(self):
        """ms of the last dispatcher wake: scan, due compaction, advance."""
        buf = (C.c_float * 12)()
        lib().cg_last_kernel_times(self._h, buf, 12)
        return list(buf)[9:12]

    def fanout_ms(self):
        """ms of the last Dispatcher.fanout (cg_last_kernel_times [13]; it
        spans the read-back of the pair total between the two passes)."""
        buf = (C.c_float * 14)()
        check(lib().cg_last_kernel_times(self._h, buf, 14))
        return float(buf[13])

    def sync(self):
        check(lib().cg_sync(self._h))

    # --------------------------------------------------------- per node
    def rule_nodes(self, rules, mode=_lib.EXCLUDE_NONE):
        rin = rules.to_c()
        nnz = C.c_int64()
        check(lib().cg_rule_nodes(self._h, C.byref(rin), mode, None, None, 0, C.byref(nnz)))
        off = np.empty(rules.n_rules + 1, dtype=np.int64)
        nodes = np.empty(max(nnz.value, 1), dtype=np.int32)
        check(lib().cg_rule_nodes(self._h, C.byref(rin), mode, off.ctypes.data, nodes.ctypes.data,
                                  nnz.value, C.byref(nnz)))
        return off, nodes[:nnz.value]

    def expand_per_node(self, specs, loc, t0, t1, rules, mode=_lib.EXCLUDE_NONE):
        sp = self._specs(specs)
        rin = rules.to_c()
        En, nnz = C.c_int64(), C.c_int64()
        check(lib().cg_expand_per_node_device(self._h, sp._h, self._loc(loc).handle, int(t0),
                                              int(t1), C.byref(rin), mode, C.byref(En),
                                              C.byref(nnz)))
        out = _lib.cg_node_csr()
        node_off = np.empty(rules.n_nodes + 1, dtype=np.int64)
        time = np.empty(max(En.value, 1), dtype=np.int64)
        rule = np.empty(max(En.value, 1), dtype=np.int32)
        out.node_off, out.time, out.rule = node_off.ctypes.data, time.ctypes.data, rule.ctypes.data
        out.cap = En.value
        check(lib().cg_expand_per_node(self._h, sp._h, self._loc(loc).handle, int(t0), int(t1),
                                       C.byref(rin), mode, C.byref(out)))
        return node_off, time[:En.value], rule[:En.value]

    def expand_per_node_device(self, specs, loc, t0, t1, rules, mode=_lib.EXCLUDE_NONE):
        rin = rules.to_c()
        En, nnz = C.c_int64(), C.c_int64()
        check(lib().cg_expand_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0),
                                              int(t1), C.byref(rin), mode, C.byref(En),
                                              C.byref(nnz)))
        return En.value, nnz.value

    def upload_rules(self, rules):
        """A rule set resident in HBM (validated once; cg_rules_upload)."""
        h = C.c_void_p()
        rin = rules.to_c()
        check(lib().cg_rules_upload(self._h, C.byref(rin), C.byref(h)))
        return DeviceRules(self, h, rules)

    def expand_per_node_rules_device(self, specs, loc, t0, t1, drules, mode=_lib.EXCLUDE_NONE):
        En, nnz = C.c_int64(), C.c_int64()
        check(lib().cg_expand_per_node_rules_device(self._h, specs._h, self._loc(loc).handle,
                                                    int(t0), int(t1), drules._h, mode,
                                                    C.byref(En), C.byref(nnz)))
        return En.value, nnz.value

    def expand_per_node_async(self, specs, loc, t0, t1, drules, mode=_lib.EXCLUDE_NONE):
        """Enqueue one per-node window (cg_expand_per_node_rules_device_async):
        the next window's expansion and records overlap this one's writer.
        Results and errors come with expand_per_node_wait()."""
        check(lib().cg_expand_per_node_rules_device_async(self._h, specs._h, self._loc(loc).handle, int(t0),
                                                          int(t1), drules._h, mode))

    def expand_per_node_wait(self, with_total=False):
        """Wait for the pipelined per-node windows; returns the last window's
        node-event total (its result is then the readable per-node result),
        and with with_total also the node events of every window waited for."""
        n, tot = C.c_int64(), C.c_int64()
        check(lib().cg_expand_per_node_wait(self._h, C.byref(n), C.byref(tot)))
        return (n.value, tot.value) if with_total else n.value

    def node_result_device(self):
        """Device pointers of the last per-node result: (node_off, time, rule, n_events)."""
        o, t, r, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().cg_node_result_device(self._h, C.byref(o), C.byref(t), C.byref(r), C.byref(n)))
        return o.value, t.value, r.value, n.value

    def node_result_tensors(self, n_nodes):
        """The last per-node result as zero-copy torch views of the engine's
        device buffers (node_off int64 [N+1], time int64 [E], rule int32 [E]),
        valid until the next per-node call (__cuda_array_interface__)."""
        import torch
        o, t, r, n = self.node_result_device()

        class _View:
            def __init__(self, ptr, count, typestr):
                self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr,
                                                 "data": (ptr, False), "version": 3}
        dev = torch.device("cuda", self.device)
        return (torch.as_tensor(_View(o, n_nodes + 1, "<i8"), device=dev),
                torch.as_tensor(_View(t, n, "<i8"), device=dev),
                torch.as_tensor(_View(r, n, "<i4"), device=dev))

    def node_result(self, n_nodes, n_events):
        """Copy the last per-node result (node_off, time, rule) to host."""
        node_off = np.empty(n_nodes + 1, dtype=np.int64)
        time = np.empty(max(n_events, 1), dtype=np.int64)
        rule = np.empty(max(n_events, 1), dtype=np.int32)
        check(lib().cg_node_result_copy(self._h, node_off.ctypes.data, time.ctypes.data,
                                        rule.ctypes.data, n_events))
        return node_off, time[:n_events], rule[:n_events]

    def node_bands(self):
        """(B, K) of the last successful synchronous per-node call, which
        pipelined windows reuse (cg_node_result_bands): every node's list is
        written in K = ceil(R / B) segments of B consecutive rules."""
        b, k = C.c_int32(), C.c_int32()
        check(lib().cg_node_result_bands(self._h, C.byref(b), C.byref(k)))
        return b.value, k.value

    def node_checksum_enqueue(self, d_nodes, k, d_out):
        """cg_node_checksum_enqueue: checksums of k nodes' lists of the last
        enqueued window (device pointers: int32 nodes [k], uint64 out [2k])."""
        check(lib().cg_node_checksum_enqueue(self._h, d_nodes, int(k), d_out))

    @staticmethod
    def node_list_checksum(time, rule):
        """The host form of cg_node_checksum_enqueue's checksums of one list."""
        def mix(x):
            x = x ^ (x >> np.uint64(30))
            x = x * np.uint64(0xBF58476D1CE4E5B9)
            x = x ^ (x >> np.uint64(27))
            x = x * np.uint64(0x94D049BB133111EB)
            return x ^ (x >> np.uint64(31))
        with np.errstate(over="ignore"):
            h = mix(np.arange(len(time), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
            ct = mix(np.asarray(time, dtype=np.int64).view(np.uint64) ^ h).sum(dtype=np.uint64)
            cr = mix(np.asarray(rule, dtype=np.int64).view(np.uint64) ^ h).sum(dtype=np.uint64)
        return int(ct), int(cr)

    def node_copy_range(self, first, count):
        """Events [first, first+count) of the last per-node result (time, rule)."""
        time = np.empty(max(count, 1), dtype=np.int64)
        rule = np.empty(max(count, 1), dtype=np.int32)
        check(lib().cg_node_result_copy_range(self._h, int(first), int(count), time.ctypes.data,
                                              rule.ctypes.data))
        return time[:count], rule[:count]

    def set_node_order(self, order):
        """Order of every node's list in later per-node calls
        (cg_set_node_order): _lib.NODE_ORDER_RULE (rule-major, the default) or
        _lib.NODE_ORDER_TIME ((time, rule), the byTime order of Cron.run,
        cron.go:64-79,220: the time-order pass runs inside every per-node call,
        pipelined windows included)."""
        check(lib().cg_set_node_order(self._h, int(order)))

    def node_order_by_time(self):
        """Reorder every node's list of the last per-node result by (time,
        rule) in device memory (cg_node_result_order_by_time; the byTime order
        of Cron.run, cron.go:64-79,220).  Returns the pass's ms."""
        check(lib().cg_node_result_order_by_time(self._h))
        buf = (C.c_float * 13)()
        lib().cg_last_kernel_times(self._h, buf, 13)
        return buf[12]

    def last_order_ms(self):
        """ms of the last time-order pass (cg_last_kernel_times [12]): the pass
        inside the last synchronous per-node call in CG_NODE_ORDER_TIME, or
        the last cg_node_result_order_by_time."""
        buf = (C.c_float * 13)()
        check(lib().cg_last_kernel_times(self._h, buf, 13))
        return buf[12]

    def node_csr_place(self, n_nodes, src_node_off, src_time, src_rule, rule_add, dst_start, dst_time, dst_rule):
        """Place one rank's per-node slice into the gathered per-node CSR on
        this engine's device (cg_node_csr_place); arguments are device
        pointers (ints), e.g. torch tensors' data_ptr()."""
        check(lib().cg_node_csr_place(self._h, int(n_nodes), C.c_void_p(src_node_off), C.c_void_p(src_time),
                                      C.c_void_p(src_rule), int(rule_add), C.c_void_p(dst_start),
                                      C.c_void_p(dst_time), C.c_void_p(dst_rule)))

    def node_csr_merge_ranks(self, n_nodes, world, run_bounds, d_time, d_rule, budget_bytes=1 << 31):
        """Merge every node's rank slices of a gathered per-node CSR into
        (time, rule) order in place (cg_node_csr_merge_ranks): run_bounds
        [n_nodes, world + 1] (host int64; run g of node n is [rb[n, g],
        rb[n, g + 1])), each run already in (time, rule) order; d_time /
        d_rule device pointers on this engine's device."""
        rb = np.ascontiguousarray(run_bounds, dtype=np.int64)
        if rb.size != n_nodes * (world + 1):
            raise ValueError("run_bounds must hold n_nodes * (world + 1) positions")
        check(lib().cg_node_csr_merge_ranks(self._h, int(n_nodes), int(world), rb.ctypes.data, C.c_void_p(d_time),
                                            C.c_void_p(d_rule), int(budget_bytes)))

    def node_counts_to_device(self, d_ptr):
        check(lib().cg_node_counts_to_device(self._h, C.c_void_p(d_ptr)))

    # ----------------------------------------------------- fire profile
    def profile(self, specs, loc, t0, width, n_buckets):
        """Fires per rule and bucket over n_buckets buckets of `width` seconds
        from t0 (cg_profile_device; bucket b is (t0 + b*width, t0 +
        (b+1)*width]): (rule_counts int32 [R, B], bucket_totals int64 [B]).
        No fire list is written; a row sums to count()'s count."""
        sp = self._specs(specs)
        B = int(n_buckets)
        check(lib().cg_profile_device(self._h, sp._h, self._loc(loc).handle, int(t0), int(width), B))
        rules = np.empty((max(sp.n, 1), B), dtype=np.int32)
        check(lib().cg_profile_copy_rules(self._h, 0, sp.n, rules.ctypes.data))
        totals = np.empty(B, dtype=np.int64)
        check(lib().cg_profile_copy_totals(self._h, totals.ctypes.data))
        return rules[:sp.n], totals

    def profile_per_node(self, specs, loc, t0, width, n_buckets, drules, mode=_lib.EXCLUDE_NONE):
        """Fires per node and bucket (cg_profile_per_node_device): int64
        [N, B], the sum of the rule counts over the rules each node runs under
        the exclude mode -- what binning expand_per_node's lists would give.
        `drules` is an uploaded rule set (upload_rules).  The rule matrix and
        totals of the same call: profile_rules() / profile_totals()."""
        B = int(n_buckets)
        check(lib().cg_profile_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width), B,
                                               drules._h, int(mode)))
        return self.profile_nodes()

    def profile_result_device(self):
        """Device pointers and shape of the last profile: (rule_counts,
        bucket_totals, node_counts or None, n_rules, n_nodes, n_buckets)."""
        r, t, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        R, N, B = C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().cg_profile_result_device(self._h, C.byref(r), C.byref(t), C.byref(n), C.byref(R), C.byref(N),
                                             C.byref(B)))
        return r.value, t.value, n.value, R.value, N.value, B.value

    def profile_rules(self, first=0, count=None):
        """Rows [first, first+count) of the last profile's rule matrix (host int32 [count, B])."""
        _, _, _, R, _, B = self.profile_result_device()
        count = R - first if count is None else int(count)
        out = np.empty((max(count, 1), B), dtype=np.int32)
        check(lib().cg_profile_copy_rules(self._h, int(first), count, out.ctypes.data))
        return out[:count]

    def profile_totals(self):
        """The last profile's bucket totals (host int64 [B])."""
        B = self.profile_result_device()[5]
        out = np.empty(B, dtype=np.int64)
        check(lib().cg_profile_copy_totals(self._h, out.ctypes.data))
        return out

    def profile_nodes(self, first=0, count=None):
        """Rows [first, first+count) of the last profile's node matrix (host int64 [count, B])."""
        _, _, _, _, N, B = self.profile_result_device()
        count = N - first if count is None else int(count)
        out = np.empty((max(count, 1), B), dtype=np.int64)
        check(lib().cg_profile_copy_nodes(self._h, int(first), count, out.ctypes.data))
        return out[:count]

    def _profile_tensors(self):
        import torch
        r, t, n, R, N, B = self.profile_result_device()

        class _View:
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr,
                                                 "data": (ptr, False), "version": 3}
        dev = torch.device("cuda", self.device)

        def view(ptr, rows, typestr, dtype):
            if rows == 0:
                return torch.zeros((0, B), dtype=dtype, device=dev)
            return torch.as_tensor(_View(ptr, (rows, B), typestr), device=dev)
        rules = view(r, R, "<i4", torch.int32)
        totals = torch.as_tensor(_View(t, (B,), "<i8"), device=dev)
        nodes = None if n is None else view(n, N, "<i8", torch.int64)
        return rules, totals, nodes

    def profile_device(self, specs, loc, t0, width, n_buckets):
        """profile() left in HBM: zero-copy torch views (rule_counts int32
        [R, B], bucket_totals int64 [B]) of the engine's profile buffers,
        valid until the next profile call (__cuda_array_interface__)."""
        check(lib().cg_profile_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                      int(n_buckets)))
        return self._profile_tensors()[:2]

    def profile_per_node_device(self, specs, loc, t0, width, n_buckets, drules, mode=_lib.EXCLUDE_NONE):
        """profile_per_node() left in HBM: torch views (rule_counts int32
        [R, B], bucket_totals int64 [B], node_counts int64 [N, B])."""
        check(lib().cg_profile_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                               int(n_buckets), drules._h, int(mode)))
        return self._profile_tensors()

    # ------------------------------------------------ in-flight profile
    @staticmethod
    def _durations(dur_ms, n):
        d = np.ascontiguousarray(dur_ms, dtype=np.int64)
        if d.shape != (n,):
            raise ValueError(f"dur_ms must hold one duration per rule ({n}), got shape {d.shape}")
        return d

    def inflight(self, specs, loc, t0, width, n_buckets, dur_ms):
        """Commands running at each bucket edge e_b = t0 + (b+1)*width, per
        rule (cg_inflight_device): (rule matrix int32 [R, B], totals int64
        [B]).  dur_ms [R]: expected run time per rule in ms (Job.AvgTime),
        rounded up to whole seconds d; cell [r, b] counts the fires t of rule
        r over (t0, t0 + B*width] with e_b - d < t <= e_b.  Commands started
        at or before t0 are not counted (the rows ramp up)."""
        sp = self._specs(specs)
        B = int(n_buckets)
        d = self._durations(dur_ms, sp.n)
        check(lib().cg_inflight_device(self._h, sp._h, self._loc(loc).handle, int(t0), int(width), B,
                                       d.ctypes.data))
        return self.profile_rules(), self.profile_totals()

    def inflight_per_node(self, specs, loc, t0, width, n_buckets, dur_ms, drules, mode=_lib.EXCLUDE_NONE):
        """Commands running per node and bucket edge (cg_inflight_per_node_device):
        int64 [N, B], the in-flight rule matrix summed over the rules each
        node runs under the exclude mode.  Rule matrix and totals of the same
        call: profile_rules() / profile_totals(); peaks: profile_node_peaks()."""
        d = self._durations(dur_ms, specs.n)
        check(lib().cg_inflight_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                                int(n_buckets), d.ctypes.data, drules._h, int(mode)))
        return self.profile_nodes()

    def inflight_device(self, specs, loc, t0, width, n_buckets, dur_ms):
        """inflight() left in HBM: torch views (rule matrix, totals), valid
        until the next profile call of either kind."""
        d = self._durations(dur_ms, specs.n)
        check(lib().cg_inflight_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                       int(n_buckets), d.ctypes.data))
        return self._profile_tensors()[:2]

    def inflight_per_node_device(self, specs, loc, t0, width, n_buckets, dur_ms, drules, mode=_lib.EXCLUDE_NONE):
        """inflight_per_node() left in HBM: torch views (rule matrix, totals,
        node matrix)."""
        d = self._durations(dur_ms, specs.n)
        check(lib().cg_inflight_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                                int(n_buckets), d.ctypes.data, drules._h, int(mode)))
        return self._profile_tensors()

    # ------------------------------------------------ admission profile
    _ADMIT_WHAT = {"admitted": _lib.PROFILE_ADMITTED, "dropped": _lib.PROFILE_DROPPED,
                   "running": _lib.PROFILE_RUNNING}

    def _admit_args(self, n, dur_ms, parallels, unit, what):
        """Checked host arrays of an admission call: (dur_ms, parallels, unit
        pointer or None, CG_PROFILE_*), plus the arrays to keep alive."""
        if what not in self._ADMIT_WHAT:
            raise ValueError(f"what must be 'admitted', 'dropped' or 'running', got {what!r}")
        d = self._durations(dur_ms, n)
        p = np.ascontiguousarray(parallels, dtype=np.int64)
        if p.shape != (n,):
            raise ValueError(f"parallels must hold one limit per rule ({n}), got shape {p.shape}")
        u = None
        if unit is not None:
            u = np.ascontiguousarray(unit, dtype=np.int32)
            if u.shape != (n,):
                raise ValueError(f"unit must hold one unit per rule ({n}), got shape {u.shape}")
        return d, p, u, self._ADMIT_WHAT[what]

    def admit(self, specs, loc, t0, width, n_buckets, dur_ms, parallels, unit=None, what="dropped"):
        """Fires Job.limit() would admit (what="admitted") or drop
        (what="dropped") per rule and bucket (cg_admit_device): (rule matrix
        int32 [R, B], totals int64 [B]).  dur_ms [R]: expected run time in ms
        (Job.AvgTime), rounded up to whole seconds d; parallels [R]: the job's
        Parallels after alone(), 0 = unlimited; unit [R] (non-decreasing, or
        None: every rule alone): rules with equal unit share one limit, and
        must share dur_ms and parallels.  A unit's fires are taken in (time,
        rule) order; one is admitted while fewer than parallels admitted
        fires a of the unit have a + d > t.  Commands started at or before t0
        are not known, so the first d seconds over-admit.  what="running":
        the commands in flight at each bucket edge e_b = t0 + (b+1)*width
        counting only the admitted fires a (e_b - d < a <= e_b) -- inflight()
        less the fires that never start; a unit's cells sum to at most its
        parallels at every edge."""
        sp = self._specs(specs)
        d, p, u, w = self._admit_args(sp.n, dur_ms, parallels, unit, what)
        check(lib().cg_admit_device(self._h, sp._h, self._loc(loc).handle, int(t0), int(width), int(n_buckets),
                                    d.ctypes.data, p.ctypes.data, None if u is None else u.ctypes.data, w))
        return self.profile_rules(), self.profile_totals()

    def admit_per_node(self, specs, loc, t0, width, n_buckets, dur_ms, parallels, unit, drules,
                       mode=_lib.EXCLUDE_NONE, what="dropped"):
        """Admitted or dropped fires per node and bucket
        (cg_admit_per_node_device): int64 [N, B], the admission rule matrix
        summed over the rules each node runs under the exclude mode -- exact
        when the rules of a unit run on the same nodes.  Rule matrix, totals,
        peaks and top rules of the same call: profile_rules() /
        profile_totals() / profile_node_peaks() / profile_top_rules()."""
        d, p, u, w = self._admit_args(specs.n, dur_ms, parallels, unit, what)
        check(lib().cg_admit_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                             int(n_buckets), d.ctypes.data, p.ctypes.data,
                                             None if u is None else u.ctypes.data, w, drules._h, int(mode)))
        return self.profile_nodes()

    def admit_device(self, specs, loc, t0, width, n_buckets, dur_ms, parallels, unit=None, what="dropped"):
        """admit() left in HBM: torch views (rule matrix, totals), valid until
        the next profile call of any kind."""
        d, p, u, w = self._admit_args(specs.n, dur_ms, parallels, unit, what)
        check(lib().cg_admit_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width), int(n_buckets),
                                    d.ctypes.data, p.ctypes.data, None if u is None else u.ctypes.data, w))
        return self._profile_tensors()[:2]

    def admit_kernel_times(self):
        """ms of the last admission call's own kernels (cg_last_kernel_times
        [19..20]): the pass that zeroes the rewritten rows, k_admit_units."""
        buf = (C.c_float * 21)()
        check(lib().cg_last_kernel_times(self._h, buf, 21))
        return list(buf)[19:21]

    # ------------------------------------------------------ lock profile
    _LOCK_WHAT = {"granted": _lib.PROFILE_LOCK_GRANTED, "skipped": _lib.PROFILE_LOCK_SKIPPED,
                  "running": _lib.PROFILE_LOCK_RUNNING}

    def _lock_args(self, n, kind, avg_time_ms, unit, contends, lock_ttl, what):
        """Checked host arrays of a lock call: (kind int32, avg_time_ms int64,
        unit int32 or None, contends uint8 or None, lock_ttl, CG_PROFILE_*)."""
        if what not in self._LOCK_WHAT:
            raise ValueError(f"what must be 'granted', 'skipped' or 'running', got {what!r}")
        k = np.ascontiguousarray(kind, dtype=np.int32)
        if k.shape != (n,):
            raise ValueError(f"kind must hold one Job.Kind per rule ({n}), got shape {k.shape}")
        a = np.ascontiguousarray(avg_time_ms, dtype=np.int64)
        if a.shape != (n,):
            raise ValueError(f"avg_time_ms must hold one AvgTime per rule ({n}), got shape {a.shape}")
        u = c = None
        if unit is not None:
            u = np.ascontiguousarray(unit, dtype=np.int32)
            if u.shape != (n,):
                raise ValueError(f"unit must hold one unit per rule ({n}), got shape {u.shape}")
        if contends is not None:
            c = np.ascontiguousarray(np.asarray(contends) != 0, dtype=np.uint8)
            if c.shape != (n,):
                raise ValueError(f"contends must hold one flag per rule ({n}), got shape {c.shape}")
        if int(lock_ttl) < 2:
            raise ValueError(f"lock_ttl must be at least 2 (conf.go:136-138), got {lock_ttl}")
        return k, a, u, c, int(lock_ttl), self._LOCK_WHAT[what]

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    def lock_runs(self, specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit=None, contends=None, lock_ttl=300,
                  what="skipped"):
        """Fires the KindAlone / KindInterval lock of Cmd.Run would grant
        (what="granted") or skip (what="skipped") per rule and bucket
        (cg_lock_profile_device): (rule matrix int32 [R, B], totals int64
        [B]).  kind [R]: Job.Kind (_lib.JOB_*); avg_time_ms [R]: Job.AvgTime
        as stored; unit [R] (non-decreasing, or None: every rule alone): the
        job, cluster-wide -- its rules share one lock and must share kind and
        avg_time_ms; contends [R] (or None: all): 0 where the rule reaches no
        lock (rule_contends); lock_ttl: conf LockTtl.  A lock unit's
        contending fires are taken in (time, rule) order: one is skipped while
        t < free_at or when its lockTtl is 0, else granted with free_at = t +
        ttl (INTERVAL) or t + ceil(AvgTime) + ttl (ALONE), ttl being
        lock_ttl_batch at now = t.  granted + skipped == profile().  Locks
        held at t0 are not known (cold start).  what="running": the commands
        in flight at each bucket edge e_b = t0 + (b+1)*width counting only the
        granted fires g (e_b - d < g <= e_b, d = ceil(max(AvgTime, 0)) for both
        kinds); rows of COMMON units and of non-contending rules are
        inflight()'s, and an ALONE unit's cells sum to at most 1."""
        sp = self._specs(specs)
        k, a, u, c, ttl, w = self._lock_args(sp.n, kind, avg_time_ms, unit, contends, lock_ttl, what)
        check(lib().cg_lock_profile_device(self._h, sp._h, self._loc(loc).handle, int(t0), int(width), int(n_buckets),
                                           k.ctypes.data, a.ctypes.data, self._ptr(u), self._ptr(c), ttl, w))
        return self.profile_rules(), self.profile_totals()

    def lock_runs_per_node(self, specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit, contends, drules,
                           mode=_lib.EXCLUDE_NONE, lock_ttl=300, what="skipped"):
        """Granted or skipped fires per node and bucket
        (cg_lock_profile_per_node_device): int64 [N, B], the lock rule matrix
        summed over the rules each node runs under the exclude mode.  The
        SKIPPED row is exact (the fires of the node's Cmds at which the job ran
        on no node); the GRANTED row is an upper bound (the fires at which the
        node contends for a free lock -- which node wins is etcd arrival
        order).  Rule matrix, totals, peaks and top rules of the same call:
        profile_rules() / profile_totals() / profile_node_peaks() /
        profile_top_rules()."""
        k, a, u, c, ttl, w = self._lock_args(specs.n, kind, avg_time_ms, unit, contends, lock_ttl, what)
        check(lib().cg_lock_profile_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                                    int(n_buckets), k.ctypes.data, a.ctypes.data, self._ptr(u),
                                                    self._ptr(c), ttl, w, drules._h, int(mode)))
        return self.profile_nodes()

    def lock_runs_device(self, specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit=None, contends=None,
                         lock_ttl=300, what="skipped"):
        """lock_runs() left in HBM: torch views (rule matrix, totals), valid
        until the next profile call of any kind."""
        k, a, u, c, ttl, w = self._lock_args(specs.n, kind, avg_time_ms, unit, contends, lock_ttl, what)
        check(lib().cg_lock_profile_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                           int(n_buckets), k.ctypes.data, a.ctypes.data, self._ptr(u), self._ptr(c),
                                           ttl, w))
        return self._profile_tensors()[:2]

    def lock_runs_per_node_device(self, specs, loc, t0, width, n_buckets, kind, avg_time_ms, unit, contends, drules,
                                  mode=_lib.EXCLUDE_NONE, lock_ttl=300, what="skipped"):
        """lock_runs_per_node() left in HBM: torch views (rule matrix, totals,
        node matrix)."""
        k, a, u, c, ttl, w = self._lock_args(specs.n, kind, avg_time_ms, unit, contends, lock_ttl, what)
        check(lib().cg_lock_profile_per_node_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(width),
                                                    int(n_buckets), k.ctypes.data, a.ctypes.data, self._ptr(u),
                                                    self._ptr(c), ttl, w, drules._h, int(mode)))
        return self._profile_tensors()

    def rule_contends(self, rules, mode=_lib.EXCLUDE_NONE):
        """uint8 [R] for a RulesIn: 1 where the rule is scheduled on some node
        under the exclude mode (rule_nodes' degree > 0), 0 where it reaches no
        lock: on no node, or replaced everywhere by a later rule with the same
        Cmd key."""
        return contends_of(self.rule_nodes(rules, mode)[0])

    def lock_kernel_times(self):
        """ms of the last lock call's own kernels (cg_last_kernel_times [19],
        [21]): the pass that zeroes the rewritten rows, k_lock_units."""
        buf = (C.c_float * 22)()
        check(lib().cg_last_kernel_times(self._h, buf, 22))
        return [buf[19], buf[21]]

    def running_kernel_times(self):
        """ms of the prefix sum along the rewritten rows of the last running
        profile, admit*(what="running") or lock_runs*(what="running")
        (cg_last_kernel_times [22], k_rows_prefix); 0 after any other kind."""
        buf = (C.c_float * 23)()
        check(lib().cg_last_kernel_times(self._h, buf, 23))
        return buf[22]

    # ---------------------------------------------------- fire verdicts
    def _verdict_args(self, n, admit, lock):
        """(cg_admit_args or None, cg_lock_args or None, arrays to keep alive)
        of a verdict call: admit = (dur_ms, parallels, unit), lock = (kind,
        avg_time_ms, unit, contends, lock_ttl)."""
        keep, a, l = [], None, None
        if admit is not None:
            dur_ms, parallels, unit = admit
            d, p, u, _ = self._admit_args(n, dur_ms, parallels, unit, "dropped")
            a = _lib.cg_admit_args(d.ctypes.data, p.ctypes.data, self._ptr(u))
            keep += [d, p, u]
        if lock is not None:
            kind, avg_time_ms, unit, contends, lock_ttl = lock
            k, av, u, c = self._lock_arrays(n, kind, avg_time_ms, unit, contends)
            l = _lib.cg_lock_args(k.ctypes.data, av.ctypes.data, self._ptr(u), self._ptr(c), int(lock_ttl))
            keep += [k, av, u, c]
        return a, l, keep

    def _lock_arrays(self, n, kind, avg_time_ms, unit, contends):
        # _lock_args without its lock_ttl check: the library's code and message are the call's
        k, a, u, c, _, _ = self._lock_args(n, kind, avg_time_ms, unit, contends, 2, "skipped")
        return k, a, u, c

    def expand_verdicts_device(self, specs, loc, t0, t1, admit=None, lock=None):
        """expand_device() plus one verdict byte per fire, left in HBM
        (cg_expand_verdicts_device): the event total.  Bit 0
        (_lib.VERDICT_DROPPED): Job.limit() would drop the fire, given admit =
        (dur_ms, parallels, unit) as admit() takes them; bit 1
        (_lib.VERDICT_SKIPPED): the KindAlone / KindInterval lock would skip
        it, given lock = (kind, avg_time_ms, unit, contends, lock_ttl) as
        lock_runs() takes them.  The two bits are independent, as the two
        profiles are.  The call replaces the engine's expansion result
        (result_device, copy_times) and leaves the profile alone."""
        a, l, keep = self._verdict_args(specs.n, admit, lock)
        n = C.c_int64()
        check(lib().cg_expand_verdicts_device(self._h, specs._h, self._loc(loc).handle, int(t0), int(t1),
                                              None if a is None else C.byref(a), None if l is None else C.byref(l),
                                              C.byref(n)))
        del keep
        self._verdict_rules = specs.n  # sel_off of a later verdicts_select has one more entry
        return n.value

    def expand_verdicts(self, specs, loc, t0, t1, admit=None, lock=None):
        """(offsets int64 [R+1], times int64 [E], verdict uint8 [E]) of
        expand_verdicts_device(), copied to the host."""
        sp = self._specs(specs)
        try:
            n = self.expand_verdicts_device(sp, loc, t0, t1, admit, lock)
            off = np.empty(sp.n + 1, dtype=np.int64)
            check(lib().cg_result_copy_offsets(self._h, off.ctypes.data))
            return off, self.copy_times(0, n), self.verdicts_copy(0, n)
        finally:
            if sp is not specs:  # uploaded here: the result does not read it
                sp.free()

    def verdicts_device(self):
        """(device pointer of the verdict bytes, event total); CgError
        (CG_EINVAL) when no verdict call succeeded or a later expansion call
        replaced its result."""
        p, n = C.c_void_p(), C.c_int64()
        check(lib().cg_verdicts_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def verdicts_copy(self, first, count):
        out = np.empty(max(count, 1), dtype=np.uint8)
        check(lib().cg_verdicts_copy(self._h, int(first), int(count), out.ctypes.data))
        return out[:count]

    def verdicts_select_device(self, mask, value):
        """Selects the fires with (verdict & mask) == value on the device
        (cg_verdicts_select_device): their count."""
        n = C.c_int64()
        check(lib().cg_verdicts_select_device(self._h, int(mask), int(value), C.byref(n)))
        return n.value

    def verdicts_selected_device(self):
        """(sel_off pointer, sel_times pointer, count) of the last selection."""
        o, t, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().cg_verdicts_selected_device(self._h, C.byref(o), C.byref(t), C.byref(n)))
        return o.value, t.value, n.value

    def verdicts_select(self, mask, value, n_rules=None):
        """(sel_off int64 [R+1], sel_times int64 [n]): the rule-major CSR of
        the fires with (verdict & mask) == value, ascending per rule.  mask 1:
        by Job.limit(), 2: by the lock, 3: both bits."""
        n = self.verdicts_select_device(mask, value)
        if n_rules is None:
            n_rules = self._verdict_rules
        off = np.empty(n_rules + 1, dtype=np.int64)
        check(lib().cg_verdicts_selected_copy_offsets(self._h, off.ctypes.data))
        times = np.empty(max(n, 1), dtype=np.int64)
        check(lib().cg_verdicts_selected_copy_times(self._h, 0, n, times.ctypes.data))
        return off, times[:n]

    def verdict_times(self):
        """ms of the last verdict call and selection (cg_verdict_times):
        expansion, init pass, admission walk, lock walk, selection count +
        scan, selection write."""
        buf = (C.c_float * 6)()
        k = lib().cg_verdict_times(self._h, buf, 6)
        return list(buf)[:max(k, 0)]

    def profile_kind(self):
        """What the readable profile holds: _lib.PROFILE_STARTS,
        PROFILE_INFLIGHT, PROFILE_ADMITTED, PROFILE_DROPPED, PROFILE_LOCK_GRANTED,
        PROFILE_LOCK_SKIPPED, PROFILE_RUNNING (commands in flight after
        Job.limit(), admit*(what="running")) or PROFILE_LOCK_RUNNING (after the
        job lock, lock_runs*(what="running")) (cg_profile_kind)."""
        k = C.c_int()
        check(lib().cg_profile_kind(self._h, C.byref(k)))
        return k.value

    def profile_node_peaks(self, first=0, count=None):
        """Per node row [first, first+count) of the last profile's node matrix
        (of either kind): (peak int64 [count], bucket int32 [count]) -- the
        largest cell and the first bucket attaining it; (0, 0) for a zero row."""
        N = self.profile_result_device()[4]
        count = N - first if count is None else int(count)
        peak = np.empty(max(count, 1), dtype=np.int64)
        bucket = np.empty(max(count, 1), dtype=np.int32)
        check(lib().cg_profile_node_peaks(self._h, int(first), count, peak.ctypes.data, bucket.ctypes.data))
        return peak[:count], bucket[:count]

    # ------------------------------------------------ top rules of a bucket
    def profile_top_rules_device(self):
        """Device pointers and shape of the last top-rules result
        (cg_profile_top_rules_device): (rule, count, n_listed, n_contrib,
        bucket, rows, k); rule / count are int32 [rows, k], the others int32
        [rows].  Valid until the next top-rules or profile call."""
        p = [C.c_void_p() for _ in range(5)]
        rows, k = C.c_int32(), C.c_int32()
        check(lib().cg_profile_top_rules_device(self._h, *[C.byref(x) for x in p], C.byref(rows), C.byref(k)))
        return tuple(x.value for x in p) + (rows.value, k.value)

    def profile_top_rules_copy(self, first=0, count=None):
        """Rows [first, first+count) of the last top-rules result on the host:
        (rule [count, k], count [count, k], n_listed, n_contrib, bucket)."""
        rows, k = self.profile_top_rules_device()[5:]
        count = rows - first if count is None else int(count)
        n = max(count, 1)
        rule, cnt = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.int32)
        nl, nc, bk = (np.empty(n, dtype=np.int32) for _ in range(3))
        check(lib().cg_profile_top_rules_copy(self._h, int(first), count, rule.ctypes.data, cnt.ctypes.data,
                                              nl.ctypes.data, nc.ctypes.data, bk.ctypes.data))
        return rule[:count], cnt[:count], nl[:count], nc[:count], bk[:count]

    def profile_top_rules(self, k, buckets=None):
        """Per node of the last per-node profile (of either kind), the rules it
        runs with the largest cells in one bucket (cg_profile_top_rules_nodes):
        (rule int32 [N, k], count int32 [N, k], n_listed [N], n_contrib [N],
        bucket [N]).  Row n ranks bucket buckets[n], by default the node's peak
        bucket (profile_node_peaks); its contributors -- rules with a cell > 0
        there -- are ordered by (count descending, rule index ascending) and
        cut to k, padded with (-1, 0)."""
        b = None
        if buckets is not None:
            N = self.profile_result_device()[4]
            b = np.ascontiguousarray(buckets, dtype=np.int32)
            if b.shape != (N,):
                raise ValueError(f"buckets must hold one bucket per node ({N}), got shape {b.shape}")
        check(lib().cg_profile_top_rules_nodes(self._h, int(k), None if b is None or b.size == 0 else b.ctypes.data))
        return self.profile_top_rules_copy()

    def profile_top_rules_bucket(self, bucket, k):
        """profile_top_rules for the one cluster-wide row: all rules of the
        last profile, each once (cg_profile_top_rules_bucket); arrays of one
        row.  Works after a profile call without a node matrix too."""
        check(lib().cg_profile_top_rules_bucket(self._h, int(bucket), int(k)))
        return self.profile_top_rules_copy()

    def profile_top_rules_ms(self):
        """Of the last top-rules call (cg_profile_top_rules_times): [device ms
        of the select, of the merge of split rows (0 when none was split), the
        number of chunks the rows were cut into]."""
        buf = (C.c_float * 3)()
        n = check(lib().cg_profile_top_rules_times(self._h, buf, 3))
        return list(buf)[:n]

    def profile_kernel_times(self):
        """ms of the last profile call (cg_last_kernel_times [14..18]):
        k_profile_rules, k_profile_walk, k_profile_totals, join + transpose
        (0 when the cached join was reused), node matrix."""
        buf = (C.c_float * 19)()
        check(lib().cg_last_kernel_times(self._h, buf, 19))
        return list(buf)[14:19]

    def fill(self, d_ptr, nbytes, byte_value=0xFF):
        """Fill a device buffer with one byte value (cg_fill_device)."""
        check(lib().cg_fill_device(self._h, C.c_void_p(d_ptr), int(nbytes), int(byte_value)))

    def fill_rates(self, d_ptr, nbytes, reps=5):
        """Store ceiling of this device over nbytes of a device buffer
        (cg_fill_rate_device): mean ms of k_fill_stream with nontemporal
        stores, with plain stores, and of hipMemsetAsync."""
        ms = (C.c_float * 3)()
        check(lib().cg_fill_rate_device(self._h, C.c_void_p(d_ptr), int(nbytes), int(reps), ms))
        return {"fill_stream_nt": ms[0], "fill_stream_plain": ms[1], "hipMemsetAsync": ms[2]}

    def count_value(self, d_ptr, n, elem_bytes=8, value=-1):
        """Elements of a device array equal to value (cg_count_value_device)."""
        out = C.c_int64()
        check(lib().cg_count_value_device(self._h, C.c_void_p(d_ptr), int(n), int(elem_bytes),
                                          int(value), C.byref(out)))
        return out.value

    def checksum(self, d_ptr, n, elem_bytes=8, first_index=0, add=0):
        """Order-sensitive checksum of a device array (cg_checksum_device);
        checksums of consecutive ranges add up mod 2^64."""
        out = C.c_uint64()
        check(lib().cg_checksum_device(self._h, C.c_void_p(d_ptr), int(n), int(elem_bytes),
                                       int(first_index), int(add), C.byref(out)))
        return out.value


_default = None
_default_lock = threading.Lock()


def contends_of(rule_node_off):
    """uint8 [R] from the offsets [R+1] of a rule->node join (Engine.rule_nodes):
    1 where the rule runs on some node, 0 where it reaches no lock."""
    return (np.diff(np.asarray(rule_node_off, dtype=np.int64)) > 0).astype(np.uint8)


def default_engine():
    global _default
    with _default_lock:
        if _default is None:
            _default = Engine(0)
        return _default


def comm_gather_plan(counts, root, budget_bytes):
    """The library's chunk plan of the per-node CSR gather
    (cg_comm_gather_plan; host only): counts [world, N] per-node event counts
    of every rank.  Returns [(n0, n1, j, k)], as shard.node_gather_plan."""
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    world, N = cnt.shape
    n = C.c_int64()
    cap = max(1, 2 * N + 16)
    while True:
        out = np.zeros((cap, 4), dtype=np.int64)
        rc = lib().cg_comm_gather_plan(cnt.ctypes.data, world, N, int(root), int(budget_bytes), out.ctypes.data,
                                       cap, C.byref(n))
        if rc == _lib.CG_ECAPACITY:
            cap = int(n.value)
            continue
        check(rc)
        return [tuple(int(x) for x in row) for row in out[:n.value]]


def device_count():
    return lib().cg_device_count()


__all__ = ["Engine", "Specs", "Dispatcher", "RulesIn", "Comm", "default_engine", "device_count", "CgError",
           "comm_gather_plan"]
