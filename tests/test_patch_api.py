"""cg_dispatcher_patch_rules at the API surface, and dispatch.ClusterState on
the host (no device): every watch event's Edit, folded into a slot -> node-set
table with the oracle's join of the patch alone, must leave every node with
the Cmds a JobSet built from scratch over the current jobs and groups gives
it."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from patch_common import random_rule, string_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cronsun_gpu.h")
LIB = os.path.join(ROOT, "cronsun_amd", "libcronsun_gpu.so")


def test_header_declares_patch_rules():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+cg_dispatcher_patch_rules\s*\(", txt)
    assert re.search(r"#define\s+CG_ABI_VERSION\s+3\b", txt)


def test_library_exports_patch_rules():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT cg_dispatcher_patch_rules\b", out)


def test_lib_binds_patch_rules():
    from cronsun_amd import _lib
    L = _lib.lib()
    assert L.cg_abi_version() == _lib.ABI_VERSION == 3
    assert "cg_dispatcher_patch_rules" in _lib.SYMBOLS
    assert L.cg_dispatcher_patch_rules.argtypes is not None


def test_python_surface():
    from cronsun_amd import dispatch, engine
    assert callable(engine.Dispatcher.patch_rules)
    for m in ("put_job", "del_job", "put_group", "del_group"):
        assert callable(getattr(dispatch.ClusterCron, m))
        assert callable(getattr(dispatch.ClusterState, m))
    assert callable(dispatch.Edit)


def test_cluster_cron_put_job_without_a_device_fails_loudly():
    """No CPU fallback: an edit needs an MI355X (where one is visible it works)."""
    from cronsun_amd import _lib, engine
    from cronsun_amd.dispatch import ClusterCron
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    js = JobSet([Job("j0", Rules=[JobRule("r0", "@every 5s", ["g"], ["n1"], [])])],
                {"g": Group("g", "", ["n0"])})
    job = Job("j1", Rules=[JobRule("r0", "@every 3s", [], ["n2"], [])])
    cc = ClusterCron(js)
    t0 = 1767225600
    if engine.device_count() > 0:
        cc.begin(t0)
        cc.put_job(job, t0)
        assert cc.effective == t0 + 3
        assert cc.wake(t0 + 3) == {"n2": [("j1", "r0")]}
        cc.close()
        return
    with pytest.raises(_lib.CgError) as e:
        cc.put_job(job, t0)
    assert e.value.code == _lib.CG_ENODEV


# ----------------------------------------------------------- ClusterState
def _fold(table, edit):
    """The Edit's patch into the slot -> node-set table, by the oracle's join
    of the patch alone."""
    if edit.patch is None:
        return
    rin = edit.patch
    assert len(edit.patch_slots) == rin.n_rules and len(set(edit.patch_slots.tolist())) == rin.n_rules
    off, rules = O.node_rules(rin, 0, np.arange(rin.n_nodes, dtype=np.int32))
    for s in edit.patch_slots:
        table[int(s)] = set()
    for n in range(rin.n_nodes):
        for p in rules[off[n]:off[n + 1]]:
            table[int(edit.patch_slots[p])].add(n)


def _check(state, table, what):
    """Per node: the live Cmds of the table == Job.Cmds from scratch."""
    fresh = state.jobset()
    assert [(fresh.jobs[j].ID, r.ID) for j, r in zip(fresh.rule_job, fresh.rules)] == \
        [c for c in state.slot_cmd if c is not None], what
    for s, c in enumerate(state.slot_cmd):
        assert c is not None or not table.get(s), (what, s)  # a vacated slot has no nodes
    total = 0
    for n, nid in enumerate(state.node_ids):
        live = {state.slot_cmd[s] for s, nodes in table.items() if n in nodes}
        exp = {(fresh.jobs[j].ID, fresh.rules[i].ID) for j in range(len(fresh.jobs)) for i in fresh.cmds(j, nid)}
        assert live == exp, (what, nid)
        total += len(exp)
    return total


def test_cluster_state_events_vs_job_cmds_from_scratch():
    from cronsun_amd.dispatch import ClusterState
    from cronsun_amd.model import Group, Job, JobSet
    jobs, groups, nodes = string_world(67, n_jobs=60, n_nodes=30)
    js = JobSet(jobs, groups)
    assert any(j.Pause for j in jobs) and any("g8" in r.GroupIDs for r in js.rules)
    state = ClusterState(js)
    rin = js.rules_in()
    assert state.node_ids == [js.node_id(i) for i in range(rin.n_nodes)]
    off, rules = O.node_rules(rin, 0, np.arange(rin.n_nodes, dtype=np.int32))
    table = {s: set() for s in range(rin.n_rules)}
    for n in range(rin.n_nodes):
        for r in rules[off[n]:off[n + 1]]:
            table[int(r)].add(n)
    assert _check(state, table, "start") > 0
    rng = np.random.default_rng(5)
    n_groups = len(groups)

    def known():
        return state.jobs[list(state.jobs)[int(rng.integers(0, len(state.jobs)))]]

    def ev_new_job(i):
        job = Job(f"new{i}", Rules=[random_rule(rng, nodes, n_groups, "@every 7s")
                                    for _ in range(int(rng.integers(1, 4)))])
        first = state.n_slots
        e = state.put_job(job)
        fresh = list(range(first, first + len(job.Rules)))
        assert e.remove_slots == [] and e.set_slots == fresh and e.patch_slots.tolist() == fresh
        assert len(e.set_schedules) == len(fresh)
        return e

    def ev_same_ids(i, timer_only=False):
        old = known()
        job = copy.deepcopy(old)
        changed = []
        for k, r in enumerate(job.Rules):
            r.Schedule = None
            if timer_only or rng.random() < 0.3:
                r.Timer = f"@every {int(rng.integers(2, 50))}s" if r.Timer != "@every 9s" else "@every 8s"
                if r.Timer != old.Rules[k].Timer:
                    changed.append(k)
            if not timer_only:
                nr = random_rule(rng, nodes, n_groups, r.Timer)
                r.GroupIDs, r.NodeIDs, r.ExcludeNodeIDs = nr.GroupIDs, nr.NodeIDs, nr.ExcludeNodeIDs
        if not timer_only:
            job.Pause = bool(rng.random() < 0.2)
        slots = list(state.slots[old.ID])
        e = state.put_job(job)
        assert e.remove_slots == [] and e.set_slots == [slots[k] for k in changed], (i, e)
        assert e.patch_slots.tolist() == slots and state.slots[job.ID] == slots
        if timer_only:
            assert changed
        return e

    def ev_other_ids(i):
        old = known()
        job = copy.deepcopy(old)
        for r in job.Rules:
            r.Schedule = None
        job.Rules.append(random_rule(rng, nodes, n_groups, "@every 11s"))  # one rule more
        old_slots, first = list(state.slots[old.ID]), state.n_slots
        e = state.put_job(job)
        fresh = list(range(first, first + len(job.Rules)))
        assert e.remove_slots == old_slots and e.set_slots == fresh
        assert e.patch_slots.tolist() == old_slots + fresh
        assert all(state.slot_cmd[s] is None for s in old_slots)
        return e

    def ev_del_job(i):
        old = known()
        slots = list(state.slots[old.ID])
        e = state.del_job(old.ID)
        assert e.remove_slots == slots and e.set_slots == [] and e.patch_slots.tolist() == slots
        assert old.ID not in state.jobs
        again = state.del_job(old.ID)  # unknown now: nothing to do
        assert again.patch is None and not again.remove_slots and not again.set_slots
        return e

    def group_slots(gid):
        return [s for j in state.jobs.values() if any(gid in r.GroupIDs for r in j.Rules)
                for s in state.slots[j.ID]]

    def ev_put_group(i, gid=None, members=None):
        gid = gid or f"g{rng.integers(0, n_groups + 1)}"  # (g<n_groups> starts out missing)
        members = members or list(rng.choice(nodes, int(rng.integers(0, 9)), replace=False))
        e = state.put_group(Group(gid, "", members))
        assert e.set_slots == [] and e.remove_slots == []
        assert ([] if e.patch is None else e.patch_slots.tolist()) == group_slots(gid)
        return e

    def ev_del_group(i, gid=None):
        gid = gid or f"g{rng.integers(0, n_groups)}"
        had = gid in state.groups
        e = state.del_group(gid)
        assert e.set_slots == [] and e.remove_slots == []
        assert ([] if e.patch is None else e.patch_slots.tolist()) == (group_slots(gid) if had else [])
        return e

    n_before = len(state.node_ids)
    script = [("new", ev_new_job), ("other-ids", ev_other_ids), ("timer-only", lambda i: ev_same_ids(i, True)),
              ("new-node", lambda i: ev_put_group(i, "g2", ["node-3", "brand-new-node"])),
              ("del-group", lambda i: ev_del_group(i, "g3")),
              ("group-back", lambda i: ev_put_group(i, "g3", ["node-1", "node-7"])),
              ("same-ids", ev_same_ids), ("del-job", ev_del_job)]
    kinds = [("new", ev_new_job), ("same-ids", ev_same_ids), ("other-ids", ev_other_ids),
             ("del-job", ev_del_job), ("put-group", ev_put_group), ("del-group", ev_del_group)]
    while len(script) < 40:
        script.append(kinds[int(rng.integers(0, len(kinds)))])
    for i, (name, ev) in enumerate(script):
        _fold(table, ev(i))
        _check(state, table, (i, name))
    assert len(state.node_ids) == n_before + 1 and state.node_ids[-1] == "brand-new-node"
    assert any("brand-new-node" == state.node_ids[n] for nodes_ in table.values() for n in nodes_)

