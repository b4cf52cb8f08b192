"""cg_dispatcher_patch_rules against the oracle and against a rebind: after
every patch the fan-out of a wake must be the oracle's Job.Cmds filter
(O.node_rules) of the WHOLE edited rule set (rule i = slot i), restricted to
the due slots -- exact, with the path forced to FILTER, then DUE, then AUTO --
and equal to what a second dispatcher gives after a fresh bind_rules of the
edited set."""
import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone
from cronsun_amd import _lib, cron, synth
from patch_common import World, random_rule, string_world

pytestmark = pytest.mark.gpu

Z = O.ZERO_TIME
T0 = 1767225600  # 2026-01-01T00:00:00Z
PATHS = (_lib.CG_FANOUT_FILTER, _lib.CG_FANOUT_DUE, _lib.CG_FANOUT_AUTO)
MODES = (_lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE)
EVERY10 = cron.Every(10 * 10**9)


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def node_major(rin, mode):
    return O.node_rules(rin, mode, np.arange(rin.n_nodes, dtype=np.int32))


def expected(nm, n_rules, due):
    """nm restricted to the due slots: (node_off, slots)."""
    off, rules = nm
    is_due = np.zeros(n_rules, dtype=bool)
    is_due[np.asarray([s for s in due if s < n_rules], dtype=np.int64)] = True
    keep = is_due[rules]
    rank = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return rank[off], rules[keep].astype(np.int32)


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


def apply_patch(eng, d, w, jobs, **kw):
    rin, slots = w.patch(jobs, **kw)
    dr = eng.upload_rules(rin)
    d.patch_rules(dr, slots)
    dr.free()
    return slots


class Logged:
    """A dispatcher whose fire / set / remove calls can be replayed on a fresh
    one (the rebind comparison)."""

    def __init__(self, eng, scheds, t0):
        self.eng, self.scheds, self.t0, self.log = eng, list(scheds), t0, []
        self.d = eng.dispatcher(self.scheds, None, t0)

    def fire(self):
        now = self.d.effective
        self.log.append(("fire", now))
        return self.d.fire(now)[0].tolist()

    def set(self, idx, scheds, now):
        self.log.append(("set", list(idx), list(scheds), now))
        self.d.set(idx, scheds, now)

    def rebound(self, rin, mode):
        """A fresh dispatcher after the same calls and a bind of rin."""
        d2 = self.eng.dispatcher(self.scheds, None, self.t0)
        for op in self.log:
            if op[0] == "fire":
                d2.fire_count(op[1])
            else:
                d2.set(op[1], op[2], op[3])
        dr = self.eng.upload_rules(rin)
        d2.bind_rules(dr, mode)
        dr.free()
        return d2


def check_vs_oracle_and_rebind(ld, w, mode, due, what):
    rin = w.pack()
    exp = expected(node_major(rin, mode), rin.n_rules, due)
    check_all_paths(ld.d, exp, what)
    d2 = ld.rebound(rin, mode)
    check_all_paths(d2, exp, (what, "rebind"))
    d2.free()
    return len(exp[1])


def _relist(w, rng, r, n_nodes, n_groups):
    w.nids[r] = rng.choice(n_nodes, int(rng.integers(0, 4)), replace=False).astype(np.int32)
    w.gids[r] = rng.integers(0, n_groups, int(rng.integers(0, 3))).astype(np.int32)
    w.ex[r] = rng.choice(n_nodes, int(rng.integers(0, 4)), replace=False).astype(np.int32)


@pytest.mark.parametrize("mode", MODES)
def test_patch_sequence_vs_rebind(eng, mode):
    """Four patches in turn on ~1000 rules over 77 nodes (repeated Cmd keys,
    paused jobs, two missing groups), dense and sparse wakes in between."""
    rin = synth.multi_rule_jobs(400, n_nodes=77, seed=51, key_choices=2)
    rin.group_exists[[1, 7]] = 0
    w = World(rin)
    R, N, G = w.n_rules, w.n_nodes, len(w.groups)
    rng = np.random.default_rng(2000 + mode)
    ld = Logged(eng, [EVERY10] * R, T0)
    dr = eng.upload_rules(rin)
    ld.d.bind_rules(dr, mode)
    dr.free()
    assert len(ld.fire()) == R  # one wake makes every slot due
    # three slots on their own period: the wakes between the dense ones are sparse
    ld.set([3, 40, R - 2], [cron.Every(7 * 10**9)] * 3, T0 + 10)
    sizes = []

    def step(what, jobs):
        due = ld.fire()
        apply_patch(eng, ld.d, w, jobs)
        pairs = check_vs_oracle_and_rebind(ld, w, mode, due, (what, "patched"))
        due2 = ld.fire()
        pairs += check_vs_oracle_and_rebind(ld, w, mode, due2, (what, "next wake"))
        sizes.extend([len(due), len(due2)])
        assert pairs > 0, what

    # 1. node / group / exclude lists of 30 jobs
    jobs = rng.choice(len(w.job_pause), 30, replace=False)
    for j in jobs:
        for r in w.rules_of(j):
            _relist(w, rng, r, N, G)
    step("lists", jobs)
    # 2. pause 5 jobs, unpause 2
    paused = [j for j, p in enumerate(w.job_pause) if p]
    running = [j for j, p in enumerate(w.job_pause) if not p]
    flip = list(rng.choice(running, 5, replace=False)) + list(rng.choice(paused, 2, replace=False))
    for j in flip:
        w.job_pause[j] ^= 1
    step("pause", flip)
    # 3. one group's membership: every job that references it
    g = next(g for g in range(G) if w.group_exists[g] and sum(g in x for x in w.gids) > 3)
    w.groups[g] = rng.choice(N, 9, replace=False).astype(np.int32)
    step("group", {w.rule_job[r] for r in range(w.n_rules) if g in w.gids[r]})
    # 4. 20 new jobs in slots past R, after set
    new = []
    for _ in range(20):
        rules = []
        for _ in range(int(rng.integers(1, 4))):
            rules.append((rng.choice(N, int(rng.integers(0, 4)), replace=False), rng.integers(0, G, 2),
                          rng.choice(N, int(rng.integers(0, 3)), replace=False), int(rng.integers(0, 2))))
        new.append(w.add_job(rules, pause=int(rng.random() < 0.1)))
    ld.set(list(range(R, w.n_rules)), [EVERY10] * (w.n_rules - R), ld.log[-1][1])
    step("new jobs", new)
    assert min(sizes) <= 3 and max(sizes) >= R - 3, sizes  # sparse and dense wakes both seen
    ld.d.free()


def _tile_rules(R, N, seed):
    """Node 0 on every rule but R // 2, node N-1 on none; every other rule on
    node 0 and 1-5 more random nodes; one job per rule."""
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
    """R = 3*4096 + 123, N = 300: node 0's row crosses the 2048-pair fan tiles
    and the 4096-pair radix tiles, node N-1 is empty.  Every slot is due, so
    each fan-out is the whole transpose of the patched join."""
    R, N = 3 * 4096 + 123, 300
    rin = _tile_rules(R, N, 5)
    w = World(rin)
    mode = _lib.EXCLUDE_NONE
    nm = node_major(rin, mode)
    assert nm[0][1] - nm[0][0] == R - 1 and nm[0][N] == nm[0][N - 1]
    assert nm[1][2047] == 2047 and nm[1][2048] == 2048  # node 0's pairs at those positions
    d = eng.dispatcher([EVERY10] * R, None, T0)
    dr = eng.upload_rules(rin)
    d.bind_rules(dr, mode)
    dr.free()
    due = d.fire(T0 + 10)[0].tolist()
    assert len(due) == R

    def check(what, jobs, **kw):
        apply_patch(eng, d, w, jobs, **kw)
        packed = w.pack()
        nm = node_major(packed, mode)
        check_all_paths(d, expected(nm, R, due), what)
        return nm

    w.nids[0] = np.array([7, 0, 298], np.int32)
    check("slot 0", [0])
    w.nids[R - 1] = np.array([298, 1], np.int32)
    check("slot R-1", [R - 1])
    w.nids[2047] = np.array([5], np.int32)          # node 0 leaves position 2047
    w.nids[2048] = np.array([0, 9, 250], np.int32)  # and stays at the next
    check("2047 / 2048", [2047, 2048])
    for r in range(4000, 4200):
        w.nids[r] = w.nids[r][w.nids[r] != 0]
    nm = check("node 0 off [4000, 4200)", range(4000, 4200))
    assert nm[0][1] - nm[0][0] == R - 1 - 200 - 1 - 1
    for r in (10, 5000, R - 2):
        w.nids[r] = np.append(w.nids[r], N - 1).astype(np.int32)
    nm = check("node N-1's first rules", [10, 5000, R - 2])
    assert nm[0][N] - nm[0][N - 1] == 3
    on17 = [r for r in range(R) if 17 in w.nids[r]]
    assert len(on17) > 20
    for r in on17:
        w.nids[r] = w.nids[r][w.nids[r] != 17]
    nm = check("node 17 emptied", on17)
    assert nm[0][18] == nm[0][17]
    for r in (1, 4096, 8191, R - 1):
        w.nids[r] = np.array([0, 3], np.int32)
    check("every slot", range(R))  # no survivors
    for r in (20, 300, 9000):
        w.nids[r] = np.array([2, 1], np.int32)
    slots = apply_patch(eng, d, w, [20, 300, 9000], descending=True)
    assert slots.tolist() == [9000, 300, 20]
    exp = expected(node_major(w.pack(), mode), R, due)
    check_all_paths(d, exp, "descending slots")
    apply_patch(eng, d, w, [])  # the empty patch changes nothing
    check_all_paths(d, exp, "empty patch")
    # and the next wake under the patched join
    due2 = d.fire(T0 + 20)[0].tolist()
    assert len(due2) == R
    check_all_paths(d, exp, "next wake")
    d.free()


def test_growth_new_nodes_and_slots_past_the_bound_set(eng):
    rin = synth.multi_rule_jobs(60, n_nodes=33, seed=71)
    w = World(rin)
    R, N = w.n_rules, w.n_nodes
    mode = _lib.EXCLUDE_NONE
    d = eng.dispatcher([EVERY10] * R, None, T0)
    dr = eng.upload_rules(rin)
    d.bind_rules(dr, mode)
    dr.free()
    # slots R .. R+4 are set; R stays a gap the patch does not name
    d.set(list(range(R, R + 5)), [EVERY10] * 5, T0)
    due = d.fire(T0 + 10)[0].tolist()
    assert len(due) == R + 5
    check_all_paths(d, expected(node_major(rin, mode), R, due), "before")  # slots past R: no nodes
    w.n_nodes = N + 5
    w.add_job([([], [], [], 0)])  # the gap, slot R: in the edited set a rule without nodes
    jobs = [w.add_job([([N, 3, N + 4], [], [], 0), ([N + 2], [0], [N + 1], 0)]),
            w.add_job([([N + 4, N + 3], [], [], 0), ([1], [], [], 0)])]
    slots = apply_patch(eng, d, w, jobs)
    assert slots.tolist() == [R + 1, R + 2, R + 3, R + 4]
    packed = w.pack()
    assert packed.n_nodes == N + 5 and packed.n_rules == R + 5
    exp = expected(node_major(packed, mode), R + 5, due)
    check_all_paths(d, exp, "grown")
    off, sl = d.fanout()
    assert len(off) == N + 6 and off[N + 5] - off[N] >= 5   # the new nodes run something
    assert R in due and R not in sl and R + 1 in sl         # the skipped slot lands on no node
    due = d.fire(T0 + 20)[0].tolist()
    check_all_paths(d, expected(node_major(packed, mode), R + 5, due), "grown, next wake")
    d.free()


def test_errors_leave_the_join_as_it_was(eng):
    rin = synth.multi_rule_jobs(60, n_nodes=33, seed=72, key_choices=2)
    w = World(rin)
    R = w.n_rules
    mode = _lib.EXCLUDE_RULE
    d = eng.dispatcher([EVERY10] * R, None, T0)
    prin, slots = w.patch([3, 4])
    patch = eng.upload_rules(prin)
    with pytest.raises(_lib.CgError) as err:  # unbound
        d.patch_rules(patch, slots)
    assert err.value.code == _lib.CG_EINVAL
    dr = eng.upload_rules(rin)
    d.bind_rules(dr, mode)
    dr.free()
    due = d.fire(T0 + 10)[0].tolist()
    exp = expected(node_major(rin, mode), R, due)
    assert len(exp[1]) > 0
    check_all_paths(d, exp, "before")
    bad = []
    a = slots.copy(); a[0] = R; bad.append(a)            # == the dispatcher's count
    a = slots.copy(); a[-1] = -1; bad.append(a)          # negative
    a = slots.copy(); a[-1] = a[0]; bad.append(a)        # the same slot twice
    for a in bad:
        with pytest.raises(_lib.CgError) as err:
            d.patch_rules(patch, a)
        assert err.value.code == _lib.CG_EINVAL and _lib.last_error()
        check_all_paths(d, exp, ("after", a.tolist()))
    d.patch_rules(patch, slots)  # the unchanged jobs: the same join
    check_all_paths(d, exp, "same jobs")
    patch.free()
    d.free()


def test_patch_does_not_poison_the_per_node_cache(eng):
    """A per-node call on A, a patch on a dispatcher bound to B (the patch's
    join runs in the ctx buffers the per-node path caches in), the same
    per-node call on A: identical offsets and checksums."""
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

    d = eng.dispatcher([EVERY10] * rb.n_rules, None, T0)
    d.bind_rules(db, _lib.EXCLUDE_NONE)
    (off1, t1_, r1), s1 = run()
    w = World(rb)
    for r in w.rules_of(5) + w.rules_of(6):
        w.nids[r] = np.array([1, 2, 3], np.int32)
    apply_patch(eng, d, w, [5, 6])
    (off2, t2_, r2), s2 = run()
    assert off1[-1] > 0 and np.array_equal(off1, off2) and s1 == s2
    assert np.array_equal(t1_, t2_) and np.array_equal(r1, r2)
    due = d.fire(T0 + 10)[0].tolist()
    check_all_paths(d, expected(node_major(w.pack(), _lib.EXCLUDE_NONE), rb.n_rules, due), "b")
    for x in (d, da, db, sp):
        x.free()


def test_cluster_cron_with_edits_vs_job_cmds(eng):
    """25 wakes of the string world with an edit of every kind in between:
    each node's list is Job.Cmds of the current jobs and groups, restricted to
    the due Cmds, in slot order."""
    from cronsun_amd.dispatch import ClusterCron
    from cronsun_amd.model import Group, Job, JobSet
    import copy
    jobs, groups, nodes = string_world(67)
    js = JobSet(jobs, groups)
    specs = [r.Timer for r in js.rules]
    loc = oracle_zone("UTC")
    oc = O.OracleCron(oracle_parse_all(specs), loc)
    t0 = synth.T0_2026 + 40 * 86400 + 600
    oc.start(t0)
    cc = ClusterCron(js, engine=eng)
    cc.begin(t0)
    st = cc.state
    rng = np.random.default_rng(3)

    def timer_of(slot):
        jid, _ = st.slot_cmd[slot]
        return st.jobs[jid].Rules[st.slots[jid].index(slot)].Timer

    def mirror(edit, now):
        for s in edit.remove_slots:
            oc.remove(s)
        for s in edit.set_slots:
            oc.set(s, oracle_parse_all([timer_of(s)])[0], now)

    def cmds_by_node():
        """node ID -> the slots of its Cmds (Job.Cmds from scratch), ascending."""
        fresh = st.jobset()
        live = [s for s, c in enumerate(st.slot_cmd) if c is not None]
        assert len(live) == fresh.n_rules
        return {nid: sorted(live[i] for j in range(len(fresh.jobs)) for i in fresh.cmds(j, nid))
                for nid in st.node_ids}

    def known(k):
        return st.jobs[list(st.jobs)[k]]

    def ev_new(now):
        return cc.put_job(Job("late", Rules=[random_rule(rng, nodes, 8, "@every 2s") for _ in range(3)]), now)

    def ev_lists_and_timer(now):
        job = copy.deepcopy(known(7))
        for r in job.Rules:
            r.Schedule = None
            r.NodeIDs = ["node-1", "node-2", "fresh-node"]
        job.Rules[0].Timer = "@every 3s" if job.Rules[0].Timer != "@every 3s" else "@every 4s"
        job.Pause = False
        e = cc.put_job(job, now)
        assert e.remove_slots == [] and e.set_slots == [st.slots[job.ID][0]]
        return e

    def ev_more_rules(now):
        job = copy.deepcopy(known(11))
        for r in job.Rules:
            r.Schedule = None
        job.Rules.append(random_rule(rng, nodes, 8, "* * * * * *"))
        job.Pause = False
        return cc.put_job(job, now)

    def ev_del(now):
        return cc.del_job(known(20).ID, now)

    edits = {2: ev_new, 5: ev_lists_and_timer, 8: ev_more_rules, 11: ev_del,
             14: lambda now: cc.put_group(Group("g8", "", ["node-0", "node-5", "node-9"]), now),  # was missing
             17: lambda now: cc.del_group("g2", now),
             20: lambda now: cc.put_group(Group("g2", "", ["node-3", "fresh-node"]), now)}
    cmds = cmds_by_node()
    total, last = 0, t0
    for wk in range(25):
        if wk in edits:
            mirror(edits[wk](last), last)
            cmds = cmds_by_node()
        e = oc.effective()
        assert cc.effective == e and e != Z, wk
        now = e + int(rng.choice([0, 0, 1, 61]))
        due = set(oc.fire(e, now))
        got = cc.wake(now)
        exp = {}
        for nid, slots in cmds.items():
            lst = [st.slot_cmd[s] for s in slots if s in due]
            if lst:
                exp[nid] = lst
        assert got == exp, wk
        total += sum(len(v) for v in exp.values())
        last = now
    assert total > 0 and "fresh-node" in st.node_ids
    cc.close()
