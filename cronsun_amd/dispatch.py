"""node/cron's Cron runner (node/cron/cron.go) over the GPU-resident
dispatcher (cg_dispatcher_*, Engine.dispatcher).

  Cron(location)            NewWithLocation (cron.go:87-100)
  AddFunc / AddJob          cron.go:110-123 (parse + Schedule)
  Schedule(schedule, job)   add or replace by Job.GetID() (cron.go:125-142)
  DelFunc / DelJob          cron.go:144-164
  Entries()                 snapshot (cron.go:166-174, 296-308), byTime order
  Start() / Stop()          the run loop in its own thread (cron.go:181-187, 287-294)
  wake(now)                 one timer wake of run() (cron.go:234-244), returns
                            the entries it ran -- the loop body, callable
                            directly for deterministic drivers and tests
  ClusterCron(jobset)       every cronnode's Cron as one table: begin(now) /
                            wake(now) -> {node ID: [(Job.ID, Rule.ID), ...]}
                            (cg_dispatcher_bind_rules + cg_dispatcher_fanout)

Entry state (schedule, Next, Prev) lives in HBM; a wake is one fused kernel
plus an ordered compaction instead of sort.Sort over every entry.  Jobs run on
Python threads, as the reference runs them on goroutines (runWithRecovery,
cron.go:189-199).  Times are whole unix seconds (Next drops nanoseconds).
"""
import logging
import threading
import time
from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np

from ._lib import EXCLUDE_NONE, ZERO_TIME
from .cron import Parse, Schedule as _Schedule

log = logging.getLogger("cronsun_amd.cron")

_TEN_YEARS = 10 * 366 * 86400


class FuncJob:
    """cron.go:102-107: a func() as a Job; its ID is the function's identity."""

    def __init__(self, f):
        self.f = f

    def GetID(self):
        return f"pointer[{id(self.f):#x}]"

    def Run(self):
        self.f()


@dataclass
class Entry:
    """cron.go:43-62"""
    ID: str
    Schedule: Any
    Next: int = ZERO_TIME
    Prev: int = ZERO_TIME
    Job: Any = None


class Cron:
    def __init__(self, location=None, engine=None):
        self._engine = engine  # resolved at Start (default_engine)
        self._loc = location
        self._mu = threading.RLock()
        self._wake_cv = threading.Condition(self._mu)
        self._slot: Dict[str, int] = {}     # indexes (cron.go:19), Entry ID -> slot
        self._entries: List[Optional[Entry]] = []  # by slot
        self._free: List[int] = []
        self._d = None                       # Dispatcher while running
        self._thread = None
        self._stopping = False
        self.running = False
        self.ErrorLog = None

    # ------------------------------------------------------------ entries
    def Location(self):
        return self._loc

    def AddFunc(self, spec, cmd):
        return self.AddJob(spec, FuncJob(cmd))

    def AddJob(self, spec, cmd):
        self.Schedule(Parse(spec), cmd)  # ParseError propagates like Go's err
        return None

    def Schedule(self, schedule: _Schedule, cmd):
        e = Entry(ID=cmd.GetID(), Schedule=schedule, Job=cmd)
        with self._mu:
            slot = self._slot.get(e.ID)
            if slot is None:
                slot = self._free.pop() if self._free else len(self._entries)
                if slot == len(self._entries):
                    self._entries.append(None)
                self._slot[e.ID] = slot
            self._entries[slot] = e
            if self.running:
                # newEntry.Next = newEntry.Schedule.Next(time.Now()) (cron.go:246-252)
                self._d.set([slot], [schedule], int(time.time()))
                self._wake_cv.notify_all()

    def DelFunc(self, cmd):
        self.DelJob(FuncJob(cmd))

    def DelJob(self, cmd):
        with self._mu:
            slot = self._slot.pop(cmd.GetID(), None)
            if slot is None:
                return
            self._entries[slot] = None
            self._free.append(slot)
            if self.running:
                self._d.remove([slot])
                self._wake_cv.notify_all()

    def Entries(self):
        """Copies of the entries, earliest Next first, zero Next last (byTime)."""
        with self._mu:
            if self.running:
                nx, pv, _ = self._d.snapshot()
            out = []
            for slot, e in enumerate(self._entries):
                if e is None:
                    continue
                n, p = (int(nx[slot]), int(pv[slot])) if self.running else (e.Next, e.Prev)
                out.append(Entry(ID=e.ID, Schedule=e.Schedule, Next=n, Prev=p, Job=e.Job))
        out.sort(key=lambda x: (x.Next == ZERO_TIME, x.Next))
        return out

    # ---------------------------------------------------------- run loop
    def begin(self, now):
        """run()'s prologue (cron.go:212-215) at `now`, without a thread."""
        with self._mu:
            if self.running:
                return
            from .engine import default_engine
            self._engine = self._engine or default_engine()
            slots = [s for s, e in enumerate(self._entries) if e is not None]
            self._d = self._engine.dispatcher([], self._loc, now)
            if slots:
                self._d.set(slots, [self._entries[s].Schedule for s in slots], now)
            self.running = True

    def wake(self, now):
        """The timer fired at `now`: run every entry whose Next is the earliest
        (cron.go:234-244).  Returns the entries run (slot order)."""
        with self._mu:
            if self._d.effective == ZERO_TIME or now < self._d.effective:
                return []
            due, _ = self._d.fire(now)
            ran = [self._entries[int(s)] for s in due]
        for e in ran:
            threading.Thread(target=self._run_with_recovery, args=(e.Job,), daemon=True).start()
        return ran

    def _run_with_recovery(self, job):
        try:
            job.Run()
        except Exception:  # cron.go:189-199: log, keep the runner alive
            (self.ErrorLog or log).exception("cron: panic running job")

    def Start(self):
        with self._mu:
            if self.running:
                return
            self.begin(int(time.time()))
            self._stopping = False
            self._thread = threading.Thread(target=self._loop, name="cron.run", daemon=True)
            self._thread.start()

    def _loop(self):
        with self._mu:
            while not self._stopping:
                eff = self._d.effective
                now = time.time()
                due_at = now + _TEN_YEARS if eff == ZERO_TIME else eff
                if now < due_at:
                    # timer.Reset(effective.Sub(now)); adds/removes/stop re-evaluate
                    self._wake_cv.wait(timeout=min(due_at - now, 3600.0))
                    continue
                self._mu.release()
                try:
                    self.wake(int(time.time()))
                finally:
                    self._mu.acquire()

    def Stop(self):
        with self._mu:
            if not self.running:
                return
            self._stopping = True
            self._wake_cv.notify_all()
            t = self._thread
        if t is not None:
            t.join()
        with self._mu:
            nx, pv, _ = self._d.snapshot()
            for slot, e in enumerate(self._entries):
                if e is not None:
                    e.Next, e.Prev = int(nx[slot]), int(pv[slot])
            self._d.free()
            self._d = None
            self.running = False
            self._thread = None


class ClusterCron:
    """Every cronnode's Cron at once: one dispatcher table over all rules of
    a model.JobSet (slot i = rule i), fanned out to nodes after each wake.
    A cronnode runs its own Cron over Job.Cmds(node, groups)
    (node/node.go:121-158); wake(now) returns what each of those run loops
    fires at that instant.  No thread: the deterministic driver, like
    Cron.begin / Cron.wake."""

    def __init__(self, jobset, location=None, mode=EXCLUDE_NONE, engine=None):
        self.jobset = jobset
        self._loc = location
        self._mode = mode
        self._engine = engine
        self._d = None
        self._rules = None

    def begin(self, now):
        """Upload the set's schedules and rules, start the table at `now`
        (cron.go:212-215) and bind the rule -> node join."""
        from .engine import default_engine
        self._engine = self._engine or default_engine()
        js = self.jobset
        self._rules = self._engine.upload_rules(js.rules_in())
        self._d = self._engine.dispatcher(js.schedules(), self._loc, now)
        self._d.bind_rules(self._rules, self._mode)
        self._node_ids = {}
        self._cmd = [(js.jobs[j].ID, r.ID) for j, r in zip(js.rule_job, js.rules)]

    @property
    def effective(self):
        return self._d.effective

    def wake(self, now):
        """The timer fired at `now`: {node ID: [(Job.ID, Rule.ID), ...]} of the
        nodes with something due, each node's Cmds in job order, then rule
        order."""
        if self._d.effective == ZERO_TIME or now < self._d.effective:
            return {}
        self._d.fire_count(now)
        node_off, slots = self._d.fanout()
        out = {}
        for n in np.flatnonzero(np.diff(node_off)):
            nid = self._node_ids.get(int(n))
            if nid is None:
                nid = self._node_ids[int(n)] = self.jobset.node_id(int(n))
            out[nid] = [self._cmd[int(s)] for s in slots[node_off[n]:node_off[n + 1]]]
        return out

    def close(self):
        if self._d is not None:
            self._d.free()
            self._d = None
        if self._rules is not None:
            self._rules.free()
            self._rules = None


def New():
    """cron.go:82-85 (the local zone: the product needs an explicit Location;
    None means UTC here)."""
    return Cron()


def NewWithLocation(location):
    return Cron(location)


__all__ = ["ClusterCron", "Cron", "Entry", "FuncJob", "New", "NewWithLocation"]
