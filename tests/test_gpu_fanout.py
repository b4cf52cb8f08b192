"""The dispatcher's node fan-out (cg_dispatcher_bind_rules / _fanout*) against
the oracle: after every wake, each node's list must be the oracle's
Job.Cmds filter of that node (O.node_rules) intersected with the oracle Cron's
due set (OracleCron.fire), node-major, slots ascending (join_model.due_filter
of the oracle's node-major lists).  Every comparison is
exact and runs with the path forced to FILTER, then DUE, then AUTO."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, random_spec
from cronsun_amd import _lib, cron, synth
from join_model import due_filter

pytestmark = pytest.mark.gpu

Z = O.ZERO_TIME
T0 = 1767225600  # 2026-01-01T00:00:00Z
PATHS = (_lib.CG_FANOUT_FILTER, _lib.CG_FANOUT_DUE, _lib.CG_FANOUT_AUTO)
MODES = (_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE)


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def node_major(rin, mode):
    """The oracle's node -> rules CSR over every node."""
    return O.node_rules(rin, mode, np.arange(rin.n_nodes, dtype=np.int32))


def check_all_paths(d, exp, what):
    exp_off, exp_slots = exp
    try:
        for path in PATHS:
            d.set_fanout_path(path)
            off, slots = d.fanout()
            assert np.array_equal(off, exp_off), (what, path)
            assert np.array_equal(slots, exp_slots), (what, path)
    finally:
        d.set_fanout_path(_lib.CG_FANOUT_AUTO)


@pytest.mark.parametrize("mode", MODES)
def test_wake_loop_vs_oracle(eng, mode):
    """60 wakes (some late) of ~1000 rules over 77 nodes: paused jobs, missing
    groups and repeated Cmd keys, every exclude mode."""
    rin = synth.multi_rule_jobs(400, n_nodes=77, seed=51, key_choices=2)
    rin.group_exists[[1, 7]] = 0  # gs[gid] missing (job.go:280-284)
    assert rin.job_pause.any() and not rin.group_exists.all()
    assert np.isin(rin.gids[:rin.gid_off[rin.n_rules]], [1, 7]).any()
    R = rin.n_rules
    rng = np.random.default_rng(1000 + mode)
    specs = [random_spec(rng) for _ in range(R)]
    scheds = [cron.Parse(s) for s in specs]
    oc = O.OracleCron(oracle_parse_all(specs), oracle_zone("UTC"))
    oc.start(T0)
    nm = node_major(rin, mode)
    drules = eng.upload_rules(rin)
    d = eng.dispatcher(scheds, None, T0)
    d.bind_rules(drules, mode)
    seen_pairs = 0
    for w in range(60):
        e = oc.effective()
        assert d.effective == e and e != Z, w
        now = e + int(rng.choice([0, 0, 0, 1, 2, 59, 700, 4000]))
        due, _ = d.fire(now)
        odue = oc.fire(e, now)
        assert [int(x) for x in due] == odue, w
        exp = due_filter(*nm, odue)
        check_all_paths(d, exp, w)
        seen_pairs += len(exp[1])
    assert seen_pairs > 0
    d.free()
    drules.free()


def _tile_rules(R, N, seed):
    """Node 0 on every rule (its list crosses the 4096-pair radix tile and the
    4096-entry dispatch tile), node N-1 on none, rule R // 2 on no node; every
    other rule on node 0 and 1-5 more random nodes."""
    from cronsun_amd.engine import RulesIn
    rng = np.random.default_rng(seed)
    lists = []
    for r in range(R):
        if r == R // 2:
            lists.append(np.zeros(0, np.int32))
            continue
        k = int(rng.integers(1, 6))
        lists.append(np.concatenate([[0], rng.choice(np.arange(1, N - 1), k, replace=False)]).astype(np.int32))
    nid_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    zero = np.zeros(R + 1, dtype=np.int64)
    return RulesIn(N, 0, R, R, group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.arange(R, dtype=np.int32),
                   nid_off=nid_off, nids=np.concatenate(lists), gid_off=zero, gids=np.zeros(0, np.int32),
                   ex_off=zero, ex=np.zeros(0, np.int32), job_pause=np.zeros(R, np.uint8))


def test_tile_edges(eng):
    """R = 3*4096 + 123 entries, N = 300 (two radix passes): wakes with a
    single slot due, then the wake where 6/7 of the table is due."""
    R, N = 3 * 4096 + 123, 300
    single = 4096 + 77
    specs = ["@every 60s" if i % 7 else "0 0 * * * *" for i in range(R)]
    specs[single] = "@every 7s"
    rin = _tile_rules(R, N, 5)
    nm = node_major(rin, _lib.EXCLUDE_NONE)
    assert nm[0][1] - nm[0][0] == R - 1 and nm[0][N] == nm[0][N - 1]
    oc = O.OracleCron(oracle_parse_all(specs), oracle_zone("UTC"))
    oc.start(T0)
    drules = eng.upload_rules(rin)
    d = eng.dispatcher([cron.Parse(s) for s in specs], None, T0)
    d.bind_rules(drules, _lib.EXCLUDE_NONE)
    sizes = []
    for w in range(12):
        e = oc.effective()
        assert d.effective == e
        due, _ = d.fire(e)
        odue = oc.fire(e, e)
        assert [int(x) for x in due] == odue
        exp = due_filter(*nm, odue)
        check_all_paths(d, exp, (w, e - T0))
        sizes.append(len(odue))
        if e == T0 + 60:
            break
    assert sizes[0] == 1 and sizes[-1] == R - (R + 6) // 7 - 1, sizes
    # the dense wake's node 0 list, by range
    off, slots = d.fanout()
    assert off[1] - off[0] > 2 * 4096
    assert np.array_equal(d.fanout_range(off[0], off[1] - off[0]), slots[off[0]:off[1]])
    assert np.array_equal(d.fanout_range(off[17], off[18] - off[17]), slots[off[17]:off[18]])
    d.free()
    drules.free()


def test_set_and_remove_after_bind(eng):
    rin = synth.multi_rule_jobs(60, n_nodes=33, seed=71)
    R, N = rin.n_rules, rin.n_nodes
    nm = node_major(rin, _lib.EXCLUDE_NONE)
    on_nodes = np.unique(nm[1])  # rules that have nodes
    replaced, removed = int(on_nodes[2]), int(on_nodes[5])
    every = cron.Every(10 * 10**9)
    drules = eng.upload_rules(rin)
    d = eng.dispatcher([every] * R, None, T0)
    # unbound: EINVAL
    d.fire_count(T0 + 10)
    with pytest.raises(_lib.CgError) as err:
        d.fanout()
    assert err.value.code == _lib.CG_EINVAL
    d.bind_rules(drules, _lib.EXCLUDE_NONE)
    past = R + 2
    d.set([past, replaced], [every, cron.Every(5 * 10**9)], T0 + 10)
    d.remove([removed])
    # no wake since the set / remove: the due list is gone
    with pytest.raises(_lib.CgError) as err:
        d.fanout()
    assert err.value.code == _lib.CG_EINVAL
    # T0 + 15: only the replaced slot fires, on the nodes it always had
    assert d.effective == T0 + 15
    due, _ = d.fire(T0 + 15)
    assert due.tolist() == [replaced]
    exp = due_filter(*nm, [replaced])
    assert len(exp[1]) > 0
    check_all_paths(d, exp, "replaced")
    # T0 + 20: everything live; the slot past the rule set is due, on no node
    due, _ = d.fire(T0 + 20)
    due = due.tolist()
    assert past in due and replaced in due and removed not in due and len(due) == R
    exp = due_filter(*nm, due)
    check_all_paths(d, exp, "all")
    off, slots = d.fanout()
    assert removed not in slots and replaced in slots and slots.max() < R
    # a too-small copy names the required size
    n = len(slots)
    buf = np.zeros(n, dtype=np.int32)
    rc = _lib.lib().cg_dispatcher_fanout_copy(d._h, None, buf.ctypes.data, n - 1)
    assert rc == _lib.CG_ECAPACITY and str(n) in _lib.last_error()
    assert _lib.lib().cg_dispatcher_fanout_copy(d._h, None, buf.ctypes.data, n) == 0
    assert np.array_equal(buf, slots)
    p_off, p_slots, p_n = d.fanout_device()
    assert p_off and p_slots and p_n == n
    # nothing can fire any more: an empty wake, zero offsets
    d.remove(list(range(R)) + [past])
    assert d.effective == Z
    assert d.fire_count(T0 + 100)[0] == 0
    check_all_paths(d, (np.zeros(N + 1, np.int64), np.zeros(0, np.int32)), "empty")
    d.free()
    drules.free()


def test_rebind(eng):
    ra = synth.multi_rule_jobs(80, n_nodes=50, seed=81, key_choices=2)
    rb = synth.multi_rule_jobs(70, n_nodes=131, seed=82)
    n = max(ra.n_rules, rb.n_rules)
    d = eng.dispatcher([cron.Every((10 if i % 3 else 20) * 10**9) for i in range(n)], None, T0)
    da, db = eng.upload_rules(ra), eng.upload_rules(rb)
    d.bind_rules(da, _lib.EXCLUDE_CUMULATIVE)
    due, _ = d.fire(T0 + 10)
    due = due.tolist()
    check_all_paths(d, due_filter(*node_major(ra, _lib.EXCLUDE_CUMULATIVE), due), "a")
    d.bind_rules(db, _lib.EXCLUDE_RULE)
    check_all_paths(d, due_filter(*node_major(rb, _lib.EXCLUDE_RULE), due), "b")
    due, _ = d.fire(T0 + 20)
    check_all_paths(d, due_filter(*node_major(rb, _lib.EXCLUDE_RULE), due.tolist()), "b2")
    # a rule set with more rules than the dispatcher has slots is refused
    big = eng.upload_rules(synth.multi_rule_jobs(400, n_nodes=50, seed=83))
    with pytest.raises(_lib.CgError) as err:
        d.bind_rules(big, _lib.EXCLUDE_NONE)
    assert err.value.code == _lib.CG_EINVAL
    with pytest.raises(_lib.CgError) as err:
        d.bind_rules(db, 3)
    assert err.value.code == _lib.CG_EINVAL
    for x in (d, da, db, big):
        x.free()


def test_bind_does_not_poison_the_per_node_cache(eng):
    """The per-node path caches the join by (rule set, mode) in the ctx buffers
    a bind builds in: a per-node call on A, a bind of B, the same per-node call
    on A -- identical offsets and checksums."""
    ra = synth.multi_rule_jobs(150, seed=91)
    rb = synth.multi_rule_jobs(90, n_nodes=40, seed=92)
    arr, _ = cron.parse_batch(synth.spec_mix(ra.n_rules, seed=9, mix=synth.MIX_LIGHT))
    sp = eng.upload_c(arr, ra.n_rules)
    da, db = eng.upload_rules(ra), eng.upload_rules(rb)
    t0, t1 = synth.T0_2026, synth.T0_2026 + 86400

    def run():
        En, _ = eng.expand_per_node_rules_device(sp, None, t0, t1, da, _lib.EXCLUDE_NONE)
        p_off, p_time, p_rule, n = eng.node_result_device()
        assert n == En
        sums = (eng.checksum(p_time, En, 8), eng.checksum(p_rule, En, 4))
        return eng.node_result(ra.n_nodes, En), sums

    (off1, t1_, r1), s1 = run()
    d = eng.dispatcher([cron.Every(10**10)] * rb.n_rules, None, T0)
    d.bind_rules(db, _lib.EXCLUDE_NONE)
    (off2, t2_, r2), s2 = run()
    assert off1[-1] > 0 and np.array_equal(off1, off2) and s1 == s2
    assert np.array_equal(t1_, t2_) and np.array_equal(r1, r2)
    # and the bound join is B's own
    due, _ = d.fire(T0 + 10)
    check_all_paths(d, due_filter(*node_major(rb, _lib.EXCLUDE_NONE), due.tolist()), "b")
    for x in (d, da, db, sp):
        x.free()


def _string_world(seed, n_jobs=120, n_nodes=40, n_groups=8):
    """Jobs with string IDs whose Rule.IDs repeat inside a job (including ""
    and " "), interned by the C++ host layer (cg_jobset)."""
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    rng = np.random.default_rng(seed)
    nodes = [f"node-{i}" for i in range(n_nodes)]
    groups = {f"g{g}": Group(f"g{g}", "", list(rng.choice(nodes, int(rng.integers(1, 12)), replace=False)))
              for g in range(n_groups)}
    specs = synth.spec_mix(n_jobs * 4, seed=seed, mix=synth.MIX_CONFIG2)
    jobs, k = [], 0
    for j in range(n_jobs):
        rules = []
        for _ in range(int(rng.integers(1, 5))):
            rid = ["", " ", "a", "b"][int(rng.integers(0, 4))]
            gids = [f"g{rng.integers(0, n_groups + 1)}" for _ in range(rng.integers(0, 3))]
            nids = list(rng.choice(nodes, int(rng.integers(0, 4)), replace=False))
            ex = list(rng.choice(nodes, int(rng.integers(0, 3)), replace=False))
            rules.append(JobRule(rid, specs[k], gids, nids, ex))
            k += 1
        jobs.append(Job(f"job{j}", Rules=rules, Pause=bool(rng.random() < 0.05)))
    return JobSet(jobs, groups), nodes


def test_cluster_cron_vs_job_cmds(eng):
    """ClusterCron.wake: every node's Cmd list is the host Job.Cmds
    (cg_jobset_cmds) over the jobs in order, restricted to the due rules."""
    from cronsun_amd.dispatch import ClusterCron
    js, nodes = _string_world(67)
    specs = [r.Timer for r in js.rules]
    oc = O.OracleCron(oracle_parse_all(specs), oracle_zone("UTC"))
    t0 = synth.T0_2026 + 40 * 86400 + 600
    oc.start(t0)
    cmds = {nid: sorted(r for j in range(len(js.jobs)) for r in js.cmds(j, nid)) for nid in nodes}
    assert sum(len(v) for v in cmds.values()) > 0
    cc = ClusterCron(js, engine=eng)
    cc.begin(t0)
    rng = np.random.default_rng(3)
    total = 0
    for w in range(25):
        e = oc.effective()
        assert cc.effective == e and e != Z
        now = e + int(rng.choice([0, 0, 1, 61]))
        due = set(oc.fire(e, now))
        got = cc.wake(now)
        exp = {}
        for nid in nodes:
            lst = [(js.jobs[js.rule_job[r]].ID, js.rules[r].ID) for r in cmds[nid] if r in due]
            if lst:
                exp[nid] = lst
        assert got == exp, w
        total += sum(len(v) for v in exp.values())
    assert total > 0
    cc.close()
