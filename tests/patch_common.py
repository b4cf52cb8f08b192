"""Helpers of the rule-patch tests (test_patch_api.py, test_gpu_patch_rules.py):
a string world like test_gpu_fanout's, and an unpacked, editable RulesIn whose
rule i is dispatcher slot i."""
import numpy as np

from cronsun_amd import synth
from cronsun_amd.engine import RulesIn
from cronsun_amd.model import Group, Job, JobRule


def string_world(seed, n_jobs=120, n_nodes=40, n_groups=8):
    """(jobs, groups, nodes): string IDs, Rule.IDs repeating inside a job
    (including "" and " "), paused jobs, rules naming the missing group
    g<n_groups>."""
    rng = np.random.default_rng(seed)
    nodes = [f"node-{i}" for i in range(n_nodes)]
    groups = {f"g{g}": Group(f"g{g}", "", list(rng.choice(nodes, int(rng.integers(1, 12)), replace=False)))
              for g in range(n_groups)}
    specs = synth.spec_mix(n_jobs * 4, seed=seed, mix=synth.MIX_CONFIG2)
    jobs, k = [], 0
    for j in range(n_jobs):
        rules = []
        for _ in range(int(rng.integers(1, 5))):
            rules.append(random_rule(rng, nodes, n_groups, specs[k]))
            k += 1
        jobs.append(Job(f"job{j}", Rules=rules, Pause=bool(rng.random() < 0.05)))
    return jobs, groups, nodes


def random_rule(rng, nodes, n_groups, timer):
    rid = ["", " ", "a", "b"][int(rng.integers(0, 4))]
    gids = [f"g{rng.integers(0, n_groups + 1)}" for _ in range(rng.integers(0, 3))]
    nids = list(rng.choice(nodes, int(rng.integers(0, 4)), replace=False))
    ex = list(rng.choice(nodes, int(rng.integers(0, 3)), replace=False))
    return JobRule(rid, timer, gids, nids, ex)


def _split(off, vals, n):
    return [np.array(vals[off[i]:off[i + 1]], dtype=np.int32) for i in range(n)]


def _join(lists):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    vals = np.concatenate(lists).astype(np.int32) if lists and off[-1] else np.zeros(0, np.int32)
    return off, vals


class World:
    """A RulesIn unpacked into per-rule and per-group lists: edit the lists,
    pack() the whole edited set (rule i = slot i), patch(jobs) cuts whole
    jobs out as a patch (same nodes and groups) plus their slots."""

    def __init__(self, rin):
        R, G = rin.n_rules, rin.n_groups
        self.n_nodes = rin.n_nodes
        self.groups = _split(rin.group_off, rin.group_nodes, G)
        self.group_exists = [int(x) for x in rin.group_exists[:G]]
        self.rule_job = [int(x) for x in rin.rule_job[:R]]
        self.nids = _split(rin.nid_off, rin.nids, R)
        self.gids = _split(rin.gid_off, rin.gids, R)
        self.ex = _split(rin.ex_off, rin.ex, R)
        self.job_pause = [int(x) for x in rin.job_pause[:rin.n_jobs]]
        self.rule_key = None if rin.rule_key is None else [int(x) for x in rin.rule_key[:R]]

    @property
    def n_rules(self):
        return len(self.rule_job)

    def rules_of(self, job):
        return [r for r, j in enumerate(self.rule_job) if j == job]

    def add_job(self, rules, pause=0):
        """rules: [(nids, gids, ex, key)] -> the new job's number; its rules
        take the next slots."""
        j = len(self.job_pause)
        self.job_pause.append(int(pause))
        for nids, gids, ex, key in rules:
            self.rule_job.append(j)
            self.nids.append(np.array(nids, dtype=np.int32))
            self.gids.append(np.array(gids, dtype=np.int32))
            self.ex.append(np.array(ex, dtype=np.int32))
            if self.rule_key is not None:
                self.rule_key.append(int(key))
        return j

    def _rules_in(self, rules, n_nodes=None):
        jobs = []
        for r in rules:
            if not jobs or jobs[-1] != self.rule_job[r]:
                jobs.append(self.rule_job[r])
        num = {j: i for i, j in enumerate(jobs)}
        assert len(num) == len(jobs), "a job's rules must be contiguous"
        group_off, group_nodes = _join(self.groups)
        nid_off, nids = _join([self.nids[r] for r in rules])
        gid_off, gids = _join([self.gids[r] for r in rules])
        ex_off, ex = _join([self.ex[r] for r in rules])
        return RulesIn(n_nodes or self.n_nodes, len(self.groups), len(rules), len(jobs),
                       rule_key=None if self.rule_key is None else
                       np.array([self.rule_key[r] for r in rules], dtype=np.int32),
                       group_off=group_off, group_nodes=group_nodes,
                       group_exists=np.array(self.group_exists, dtype=np.uint8),
                       rule_job=np.array([num[self.rule_job[r]] for r in rules], dtype=np.int32),
                       nid_off=nid_off, nids=nids, gid_off=gid_off, gids=gids, ex_off=ex_off, ex=ex,
                       job_pause=np.array([self.job_pause[j] for j in jobs], dtype=np.uint8))

    def pack(self):
        return self._rules_in(list(range(self.n_rules)))

    def patch(self, jobs, descending=False):
        """Whole jobs as a patch: (RulesIn, slots).  descending: the jobs in
        descending order (slots descend from job to job)."""
        jobs = sorted(set(int(j) for j in jobs), reverse=descending)
        by_job = {}
        for r, j in enumerate(self.rule_job):
            by_job.setdefault(j, []).append(r)
        rules = [r for j in jobs for r in by_job.get(j, [])]
        return self._rules_in(rules), np.array(rules, dtype=np.int64)
