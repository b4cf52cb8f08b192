"""Bulk ingestion of cronsun's etcd values: the JSON of
every key under /cronsun/group/ and /cronsun/cmd/ decoded, validated and
interned in C++ (cg_jobset_ingest_*, cronsun_amd/csrc/cg_ingest.cpp), the
batch form of GetGroups("") + GetJobs() (group.go:39-63, job.go:339-365).

  js = EtcdJobSet(job_docs, group_docs, threads=16)
  js.job_status, js.group_status     per value: INGEST_OK / UNMARSHAL / ...
  js.schedules_c()                   JobRule.Schedule per rule (cg_schedule[])
                                     -> Engine.upload_c for the GPU paths
  js.rules_in()                      the interned CSR for the per-node paths
  js.job_meta()                      Kind, AvgTime, Parallels per job
  js.lock_ttls(now, ...)             Cmd.lockTtl per rule on the GPU
  js.node_inflight(t0, width, n_buckets)
                                     commands running per node and bucket edge
  js.node_drops(t0, width, n_buckets)
                                     fires Job.limit() would drop per node and bucket
  js.node_lock_skips(t0, width, n_buckets)
                                     fires at which an exclusive job ran nowhere, per node and bucket
  js.job_lock_runs(t0, width, n_buckets)
                                     per exclusive job: runs and skipped fires per bucket
  js.node_peak_rules(t0, width, n_buckets, k)
                                     per node: peak, bucket, its top k rules there
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .model import (_Interned, admission_units, drops_of, durations_of, job_lock_running_of, job_lock_runs_of,
                    lock_skips_of, peak_rules_of)


def _docs_array(docs):
    docs = [d if isinstance(d, (bytes, bytearray)) else d.encode() for d in docs]
    ptrs = (C.c_char_p * max(len(docs), 1))(*docs)
    lens = np.array([len(d) for d in docs] or [0], dtype=np.uint64)
    return docs, ptrs, lens


class EtcdJobSet(_Interned):
    def __init__(self, job_docs, group_docs=(), threads=16):
        L = lib()
        h = C.c_void_p()
        check(L.cg_jobset_new(C.byref(h)))
        self._h = h
        keep_g, gp, gl = _docs_array(group_docs)
        self.group_status = np.zeros(max(len(keep_g), 1), dtype=np.int32)
        check(L.cg_jobset_ingest_groups(h, C.cast(gp, C.c_void_p), gl.ctypes.data, len(keep_g),
                                        threads, self.group_status.ctypes.data))
        self.group_status = self.group_status[:len(keep_g)]
        keep_j, jp, jl = _docs_array(job_docs)
        self.job_status = np.zeros(max(len(keep_j), 1), dtype=np.int32)
        check(L.cg_jobset_ingest_jobs(h, C.cast(jp, C.c_void_p), jl.ctypes.data, len(keep_j),
                                      threads, self.job_status.ctypes.data))
        self.job_status = self.job_status[:len(keep_j)]
        c = _lib.cg_rules_in()
        check(L.cg_jobset_rules(h, C.byref(c)))
        self.n_rules, self.n_jobs, self.n_nodes, self.n_groups = (c.n_rules, c.n_jobs, c.n_nodes,
                                                                  c.n_groups)

    def schedules_c(self):
        """ctypes array of cg_schedule, rule order (for Engine.upload_c)."""
        arr = (_lib.cg_schedule * max(self.n_rules, 1))()
        check(lib().cg_jobset_schedules(self._h, C.cast(arr, C.c_void_p), self.n_rules))
        return arr

    def job_meta(self):
        kind = np.zeros(max(self.n_jobs, 1), dtype=np.int32)
        avg = np.zeros(max(self.n_jobs, 1), dtype=np.int64)
        par = np.zeros(max(self.n_jobs, 1), dtype=np.int64)
        check(lib().cg_jobset_job_meta(self._h, kind.ctypes.data, avg.ctypes.data, par.ctypes.data,
                                       self.n_jobs))
        n = self.n_jobs
        return kind[:n], avg[:n], par[:n]

    def job_id(self, j):
        v = lib().cg_jobset_job_id(self._h, j)
        return None if v is None else v

    def group_id(self, g):
        return lib().cg_jobset_group_id(self._h, g)

    def rule_id(self, r):
        v = lib().cg_jobset_rule_id(self._h, r)
        return None if v is None else v

    def lock_ttls(self, now, loc=None, lock_ttl=300, engine=None):
        """Cmd.lockTtl (job.go:194-233) for every rule at `now`, on the GPU."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg, _ = self.job_meta()
        rj = self.rules_in().rule_job[:self.n_rules]
        sp = eng.upload_c(self.schedules_c(), self.n_rules)
        return eng.lock_ttl_batch(sp, loc, now, kind[rj], avg[rj], lock_ttl)

    def rule_durations(self):
        """(dur_ms int64 [n_rules], rules without an estimate), as JobSet.rule_durations."""
        avg = self.job_meta()[1]
        return durations_of(avg[self.rules_in().rule_job[:self.n_rules]])

    def rule_parallels(self):
        """int64 [n_rules]: each rule's job's Parallels after alone(), as JobSet.rule_parallels."""
        par = self.job_meta()[2]
        return np.maximum(par[self.rules_in().rule_job[:self.n_rules]], 0).astype(np.int64)

    def node_drops(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None, what="dropped"):
        """Fires Job.limit() would drop per node and bucket: ({node ID: int64
        [n_buckets]}, the IDs of the jobs that were split), as JobSet.node_drops."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        dur, _ = self.rule_durations()
        unit, split = admission_units(rin, mode)
        specs = eng.upload_c(self.schedules_c(), self.n_rules)
        return drops_of(self, eng, specs, rin, t0, width, n_buckets, dur, self.rule_parallels(), unit, loc, mode,
                        what), [self.job_id(j).decode() for j in split]

    def node_running(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None):
        """Commands running per node at each bucket edge counting only the fires
        Job.limit() lets start: ({node ID: int64 [n_buckets]}, the IDs of the
        jobs that were split), as JobSet.node_running."""
        return self.node_drops(t0, width, n_buckets, loc, mode, engine, what="running")

    def job_lock_running(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """{job ID: int64 [n_buckets]} for the exclusive jobs, cluster-wide: the
        job's commands running at each bucket edge counting only the fires that
        find its lock free, as JobSet.job_lock_running."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return job_lock_running_of(eng, eng.upload_c(self.schedules_c(), self.n_rules), self.rules_in(), t0, width,
                                   n_buckets, kind, avg, loc, mode, lock_ttl, lambda j: self.job_id(j).decode())

    def rule_kinds(self):
        """(kind int32 [n_rules], avg_time_ms int64 [n_rules]), as JobSet.rule_kinds."""
        kind, avg, _ = self.job_meta()
        rj = self.rules_in().rule_job[:self.n_rules]
        return kind[rj].astype(np.int32), avg[rj].astype(np.int64)

    def node_lock_skips(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None,
                        what="skipped"):
        """Fires per node and bucket at which a KindAlone / KindInterval job
        ran on no node: {node ID: int64 [n_buckets]}, as JobSet.node_lock_skips."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return lock_skips_of(self, eng, eng.upload_c(self.schedules_c(), self.n_rules), self.rules_in(), t0, width,
                             n_buckets, kind, avg, loc, mode, lock_ttl, what)

    def job_lock_runs(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, lock_ttl=300, engine=None):
        """{job ID: (granted [n_buckets], skipped [n_buckets])} for the
        exclusive jobs, cluster-wide, as JobSet.job_lock_runs."""
        from .engine import default_engine
        eng = engine or default_engine()
        kind, avg = self.rule_kinds()
        return job_lock_runs_of(eng, eng.upload_c(self.schedules_c(), self.n_rules), self.rules_in(), t0, width,
                                n_buckets, kind, avg, loc, mode, lock_ttl, lambda j: self.job_id(j).decode())

    def node_inflight(self, t0, width, n_buckets, loc=None, mode=_lib.EXCLUDE_NONE, engine=None):
        """Commands running per node at each bucket edge, each rule running
        for its job's AvgTime: ({node ID: int64 [n_buckets]}, rules without an
        estimate), as JobSet.node_inflight."""
        from .engine import default_engine
        eng = engine or default_engine()
        rin = self.rules_in()
        dur, missing = self.rule_durations()
        specs = eng.upload_c(self.schedules_c(), self.n_rules)
        drules = eng.upload_rules(rin)
        try:
            counts = eng.inflight_per_node(specs, loc, t0, width, n_buckets, dur, drules, mode)
        finally:
            drules.free()
            specs.free()
        return {self.node_id(n): counts[n] for n in range(rin.n_nodes)}, missing

    def node_peak_rules(self, t0, width, n_buckets, k=10, inflight=False, loc=None, mode=_lib.EXCLUDE_NONE,
                        engine=None, running=False):
        """Which rules make up each node's peak: {node ID: (peak, bucket,
        [(job ID, rule ID, count), ...])}, with inflight=True (that, rules
        without an estimate), with running=True (that, the IDs of the jobs that
        were split), as JobSet.node_peak_rules."""
        from .engine import default_engine
        eng = engine or default_engine()
        if inflight and running:
            raise ValueError("inflight and running are two profiles: choose one")
        rin = self.rules_in()
        dur, missing = self.rule_durations() if inflight or running else (None, 0)
        unit, split = admission_units(rin, mode) if running else (None, [])
        res = peak_rules_of(self, eng, eng.upload_c(self.schedules_c(), self.n_rules), rin, t0, width,
                            n_buckets, k, dur, loc, mode, lambda j: self.job_id(j).decode(),
                            lambda r: self.rule_id(r).decode(), (self.rule_parallels(), unit) if running else None)
        if running:
            return res, [self.job_id(j).decode() for j in split]
        return (res, missing) if inflight else res


__all__ = ["EtcdJobSet"]
