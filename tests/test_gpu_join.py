"""The rule -> node join (k_rule_nodes), its radix transpose (k_rs_hist /
k_rs_scatter, k_node_bounds) and what stands on them -- per-node lists, the
dispatcher's fan-out and patch, the per-node profile -- against the host model
(join_model.py, pinned to the oracle by test_join_model.py) at the node counts
where the kernels change path: bitmap words past one 64-lane trip (N > 2048),
radix pass counts (N = 256 | 257, 65536 | 65537), waves per block (131072,
174752, 262144 nodes; half that with repeated Cmd keys), the 64 KiB LDS limits
and their CG_ERANGE refusals, rules past the 4096-block grid cap.  Every
comparison is exact, on whole arrays."""
import numpy as np
import pytest

import join_model as JM
from cronsun_amd import _lib, cron
from join_cases import edge_rules, nid_rules
from patch_common import World

pytestmark = pytest.mark.gpu

T0 = 1767225600  # 2026-01-01T00:00:00Z
HOUR = 3600
PATHS = (_lib.CG_FANOUT_FILTER, _lib.CG_FANOUT_DUE, _lib.CG_FANOUT_AUTO)
NONE, RULE, CUMULATIVE = _lib.EXCLUDE_NONE, _lib.EXCLUDE_RULE, _lib.EXCLUDE_CUMULATIVE
MODES = (NONE, RULE, CUMULATIVE)
EVERY1S, EVERY30M, EVERY1H = cron.Every(10**9), cron.Every(1800 * 10**9), cron.Every(HOUR * 10**9)
R_EDGE = 600
MAX_NODES, MAX_NODES_DUP = 524288, 262144  # 64 KiB of LDS: one bitmap, or two with repeated Cmd keys


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


_sets, _models, _specs = {}, {}, {}


def case(N, keys, R=R_EDGE, per=(1, 4)):
    """edge_rules(N, R, keys) built once per module: (key, RulesIn, info)."""
    key = (N, keys, R, per)
    if key not in _sets:
        _sets[key] = edge_rules(N, R, keys, seed=1000 + N % 977 + keys, rules_per_job=per)
    return (key,) + _sets[key]


def model(key, rin, mode):
    """The host model's join of a cached set, computed once per mode."""
    if (key, mode) not in _models:
        _models[key, mode] = JM.join(rin, mode)
    return _models[key, mode]


def hourly(eng, R):
    """R `@every 1h` specs in HBM: over (T0, T0 + 1h] every rule fires once,
    at T0 + 1h, so a per-node result is the transpose itself."""
    if R not in _specs:
        _specs[R] = eng.upload([EVERY1H] * R)
    return _specs[R]


def check_rule_nodes(eng, rin, mode, m):
    off, nodes = eng.rule_nodes(rin, mode)
    assert np.array_equal(off, m[0])
    assert np.array_equal(nodes, m[1])


def check_node_lists(got, m):
    node_off, time, rule = got
    assert np.array_equal(node_off, m[2])
    assert np.array_equal(rule, m[3])
    assert len(time) == len(m[3]) and (time == T0 + HOUR).all()


def check_per_node(eng, rin, mode, m):
    check_node_lists(eng.expand_per_node(hourly(eng, rin.n_rules), None, T0, T0 + HOUR, rin, mode), m)


def check_per_node_device(eng, drules, mode, m, calls=2):
    """The device-resident path; the second call takes the cached join."""
    for _ in range(calls):
        En, nnz = eng.expand_per_node_rules_device(hourly(eng, drules.n_rules), None, T0, T0 + HOUR, drules, mode)
        assert En == nnz == len(m[3])
        check_node_lists(eng.node_result(drules.n_nodes, En), m)


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


def check_ranges(d, nodes):
    off, slots = d.fanout()
    for n in nodes:
        assert np.array_equal(d.fanout_range(off[n], off[n + 1] - off[n]), slots[off[n]:off[n + 1]]), n


def bound(eng, rin, mode, scheds):
    d = eng.dispatcher(scheds, None, T0)
    dr = eng.upload_rules(rin)
    d.bind_rules(dr, mode)
    dr.free()
    return d


def check_dense_wake(eng, rin, mode, m, extra_slots=0):
    """bind_rules and the wake that makes every slot due: the fan-out is the
    whole transpose."""
    n = rin.n_rules + extra_slots
    d = bound(eng, rin, mode, [EVERY1S] * n)
    due = d.fire(T0 + 1)[0]
    assert len(due) == n
    check_all_paths(d, (m[2], m[3]), "dense")
    d.free()


def raises_erange(fn):
    with pytest.raises(_lib.CgError) as err:
        fn()
    assert err.value.code == _lib.CG_ERANGE, err.value
    assert "nodes" in str(err.value)


# ---------------------------------------------------------------- a. the sweep

@pytest.mark.parametrize("keys", [0, 2])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 256, 257, 2047, 2048, 2049, 4097, 65536, 65537])
def test_join_and_transpose_sweep(eng, N, keys):
    """One, two and three radix passes; one and several 64-word trips of the
    count and compaction loops; every exclude mode; host arrays and, once per
    set, the device-resident rule set called twice."""
    key, rin, _ = case(N, keys)
    for mode in MODES:
        m = model(key, rin, mode)
        assert m[2][1] > m[2][0] and m[2][N] > m[2][N - 1]  # nodes 0 and N-1 run something
        check_rule_nodes(eng, rin, mode, m)
        check_per_node(eng, rin, mode, m)
    dr = eng.upload_rules(rin)
    check_per_node_device(eng, dr, RULE, model(key, rin, RULE))
    dr.free()


# ------------------------------------------- b. LDS and waves-per-block edges

LDS_EDGES = [(0, n) for n in (131072, 131073, 174752, 174753, 262144, 262145, MAX_NODES)] + \
            [(2, n) for n in (65537, 87360, 87361, 131072, 131073, MAX_NODES_DUP)]


@pytest.mark.parametrize("keys,N", LDS_EDGES)
def test_waves_per_block_edges(eng, keys, N):
    """4, 3, 2 waves and one wave per block on either side of each step, up
    to the launch that asks for the whole 64 KiB of dynamic LDS."""
    key, rin, _ = case(N, keys)
    assert (rin.rule_key is not None) == bool(keys)
    limit = N == (MAX_NODES_DUP if keys else MAX_NODES)
    for mode in (CUMULATIVE, NONE) if limit else (CUMULATIVE,):
        m = model(key, rin, mode)
        check_rule_nodes(eng, rin, mode, m)
        check_per_node(eng, rin, mode, m)
    dr = eng.upload_rules(rin)
    check_per_node_device(eng, dr, CUMULATIVE, model(key, rin, CUMULATIVE))
    dr.free()


def test_keys_that_never_repeat_take_the_single_bitmap(eng):
    """rule_key with no key twice in a job: no second bitmap, so 524288 nodes
    are accepted and the join is the keyless one."""
    key, rin, _ = case(MAX_NODES, 0)
    m = model(key, rin, CUMULATIVE)
    rin.rule_key = np.arange(rin.n_rules, dtype=np.int32)
    try:
        check_rule_nodes(eng, rin, CUMULATIVE, m)
        check_per_node(eng, rin, CUMULATIVE, m)
    finally:
        rin.rule_key = None


@pytest.mark.parametrize("keys,N", [(0, MAX_NODES + 1), (2, MAX_NODES_DUP + 1)])
def test_refusals_past_the_node_limits(eng, keys, N):
    """CG_ERANGE from rule_nodes, the per-node and profile calls and bind_rules; after each
    the device-resident set that ran before gives its earlier lists again (a
    failed join leaves no stale per-node cache) and the dispatcher is unbound."""
    key, rin, _ = case(N, keys)
    skey, small, _ = case(65537, 2)
    m = model(skey, small, RULE)
    R = small.n_rules
    ds = eng.upload_rules(small)
    check_per_node_device(eng, ds, RULE, m, calls=1)
    raises_erange(lambda: eng.rule_nodes(rin, NONE))
    check_per_node_device(eng, ds, RULE, m, calls=1)
    raises_erange(lambda: eng.expand_per_node(hourly(eng, R), None, T0, T0 + HOUR, rin, NONE))
    check_per_node_device(eng, ds, RULE, m)
    big = eng.upload_rules(rin)
    raises_erange(lambda: eng.expand_per_node_rules_device(hourly(eng, R), None, T0, T0 + HOUR, big, CUMULATIVE))
    check_per_node_device(eng, ds, RULE, m)
    raises_erange(lambda: eng.profile_per_node(hourly(eng, R), None, T0, HOUR, 1, big, RULE))
    check_per_node_device(eng, ds, RULE, m)
    d = eng.dispatcher([EVERY1S] * R, None, T0)
    d.bind_rules(ds, RULE)
    d.fire(T0 + 1)
    check_all_paths(d, (m[2], m[3]), "before")
    raises_erange(lambda: d.bind_rules(big, NONE))
    with pytest.raises(_lib.CgError) as err:  # nothing is bound after the refusal
        d.fanout()
    assert err.value.code == _lib.CG_EINVAL
    check_per_node_device(eng, ds, RULE, m)
    d.bind_rules(ds, RULE)
    check_all_paths(d, (m[2], m[3]), "rebound")
    for x in (d, ds, big):
        x.free()


# ------------------------------------------------ c. rules past the grid cap

R_CAP = 4 * 4096 + 77


@pytest.mark.parametrize("per", [(6, 12), (2, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_rules_past_the_grid_cap_with_one_key(eng, mode, per):
    """R > 4096 blocks x 4 waves, every rule of a job on one Cmd key: a wave
    that takes a second rule in its stride loop starts from a used shadow
    bitmap.  With two rules a job the rule 4 x 4096 before a job's last rule
    is a job's last rule too, so every such wave has swept a key before."""
    key, rin, info = case(40, 1, R_CAP, per)
    m = model(key, rin, mode)
    assert rin.n_rules == R_CAP and m[0][-1] > R_CAP
    check_rule_nodes(eng, rin, mode, m)
    check_per_node(eng, rin, mode, m)


def test_rules_past_the_grid_cap_three_waves(eng):
    """The same R at 131073 nodes (3 waves per block: 3 x 4096 < R), 0-3
    NodeIDs a rule."""
    N = 131073
    rng = np.random.default_rng(77)
    lists = [rng.integers(0, N, int(rng.integers(0, 4))) for _ in range(R_CAP)]
    lists[0], lists[3 * 4096], lists[R_CAP - 1] = [0, N - 1], [N - 1, 2048, 0], [N - 1]
    rin = nid_rules(N, lists)
    m = JM.join(rin, NONE)
    check_rule_nodes(eng, rin, NONE, m)
    check_per_node(eng, rin, NONE, m)


# --------------------------------------------------------- d. degenerate sizes

def through_everything(eng, rin, mode=NONE):
    m = JM.join(rin, mode)
    check_rule_nodes(eng, rin, mode, m)
    check_per_node(eng, rin, mode, m)
    dr = eng.upload_rules(rin)
    check_per_node_device(eng, dr, mode, m)
    dr.free()
    check_dense_wake(eng, rin, mode, m, extra_slots=2)
    return m


def test_no_rules_and_no_pairs(eng):
    m = through_everything(eng, nid_rules(5, []))
    assert len(m[0]) == 1 and m[2].tolist() == [0] * 6
    key, rin, _ = case(300, 2)
    paused = World(rin)
    paused.job_pause = [1] * len(paused.job_pause)
    for mode in MODES:
        m = through_everything(eng, paused.pack(), mode)
        assert m[0][-1] == 0 and len(m[0]) == rin.n_rules + 1


@pytest.mark.parametrize("nnz", [2048, 2049, 4096, 4097])
def test_pair_counts_at_the_tile_edges(eng, nnz):
    """nnz on either side of the fan-out tile (2048 pairs) and the radix tile
    (4096 pairs): the last rule's NodeIDs are trimmed to fit."""
    N = 3000
    rng = np.random.default_rng(5)
    lists = [rng.choice(N, int(rng.integers(0, 5)), replace=False) for _ in range(900)]
    lists.append(rng.permutation(N))
    have = sum(len(x) for x in lists[:-1])
    assert have < 2048 and have + N > 4097
    lists[-1] = lists[-1][:nnz - have]
    m = through_everything(eng, nid_rules(N, lists))
    assert m[0][-1] == nnz


def test_one_node_on_every_rule_three_passes(eng):
    """N = 65537, every pair on one node: in each of the three radix passes
    all pairs share the digit, so a whole wave is one ballot group."""
    for node in (65536, 0):
        rin = nid_rules(65537, [[node]] * 5000)
        m = through_everything(eng, rin)
        assert m[2][node + 1] - m[2][node] == 5000 and m[3].tolist() == list(range(5000))


# ------------------------------------------------------ e. fan-out at large N

@pytest.mark.parametrize("N", [257, 2049, 65537])
def test_fanout_sparse_and_dense(eng, N):
    key, rin, _ = case(N, 2)
    R = rin.n_rules
    m = model(key, rin, RULE)
    d = bound(eng, rin, RULE, [EVERY1S if r % 5 == 0 else EVERY1H for r in range(R)])
    due = d.fire(T0 + 1)[0].tolist()
    assert due == list(range(0, R, 5))
    exp = JM.due_filter(m[2], m[3], due)
    assert 0 < len(exp[1]) < len(m[3]) // 3
    check_all_paths(d, exp, "sparse")
    empty = np.flatnonzero(np.diff(exp[0]) == 0)
    assert len(empty) > 0
    check_ranges(d, [0, N - 1, int(empty[len(empty) // 2])])
    d.set(list(range(R)), [EVERY1S] * R, T0 + 1)
    assert len(d.fire(T0 + 2)[0]) == R
    check_all_paths(d, (m[2], m[3]), "dense")
    check_ranges(d, [0, N - 1, N // 2])
    d.free()


# -------------------------------------------------------- f. patch at large N

def _relist(w, rng, r, lo, hi):
    w.nids[r] = rng.integers(lo, hi, int(rng.integers(0, 4))).astype(np.int32)
    w.ex[r] = rng.integers(lo, hi, int(rng.integers(0, 3))).astype(np.int32)


def _job_of(w, r):
    return w.rule_job[r]


class Patched:
    """A bound dispatcher, the World it is edited through and the model's
    rule set after every patch so far."""

    def __init__(self, eng, rin, mode, extra_slots):
        self.eng, self.mode, self.rin = eng, mode, rin
        self.w = World(rin)
        self.n = rin.n_rules + extra_slots
        self.sparse = [EVERY1S if r % 5 == 0 else EVERY1H for r in range(self.n)]
        self.d = bound(eng, rin, mode, self.sparse)
        self.now = T0

    def wake(self, dense):
        """Set every slot for a dense or a sparse wake, then fire it."""
        self.d.set(list(range(self.n)), [EVERY1S] * self.n if dense else self.sparse, self.now)
        self.now += 1
        due = self.d.fire(self.now)[0].tolist()
        assert due == (list(range(self.n)) if dense else list(range(0, self.n, 5)))
        return due

    def patch(self, jobs):
        prin, slots = self.w.patch(jobs)
        dr = self.eng.upload_rules(prin)
        self.d.patch_rules(dr, slots)
        dr.free()
        self.rin = JM.patched(self.rin, prin, slots)
        m = JM.join(self.rin, self.mode)
        # the model's patched set is the edited World itself
        assert all(np.array_equal(a, b) for a, b in zip(m, JM.join(self.w.pack(), self.mode)))
        return slots, m

    def check(self, m, due, what):
        check_all_paths(self.d, JM.due_filter(m[2], m[3], due), what)


@pytest.mark.parametrize("mode,N,Nn", [(mode, N, Nn) for mode in (NONE, CUMULATIVE)
                                       for N, Nn in ((250, 300), (2040, 2100), (65530, 65600))])
def test_patch_then_grow(eng, mode, N, Nn):
    """A patch of 40 slots at N nodes, then one that brings nodes up to Nn:
    the removed pairs sort with N's pass count, the delta with Nn's."""
    key, rin, info = case(N, 2)
    R = rin.n_rules
    rng = np.random.default_rng(N)
    p = Patched(eng, rin, mode, extra_slots=4)
    w = p.w
    due = p.wake(dense=False)
    p.check(model(key, rin, mode), due, "bound, sparse")
    # 1. 40 slots: the all-nodes job, the job without nodes, the key chain, two
    #    emptied slots, synthetic jobs, and three slots past R behind a gap
    a1, a2 = info["all_nodes"]
    w.nids[a1], w.gids[a1] = np.array([N - 1, 0, 7 % N], np.int32), np.zeros(0, np.int32)
    w.ex[a2] = np.array([0, N - 1, N + 5], np.int32)
    for r in info["empty"]:
        w.nids[r] = rng.integers(0, N, 70).astype(np.int32)
    for r in info["chain"]:
        _relist(w, rng, r, 0, N)
    emptied = (info["first"], info["big_group"])
    for r in emptied:
        w.nids[r], w.gids[r] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    jobs = {_job_of(w, r) for r in (a1,) + info["empty"] + info["chain"] + emptied}
    n_slots = sum(len(w.rules_of(j)) for j in jobs)
    for j in rng.permutation(_job_of(w, info["first"])):
        rules = w.rules_of(j)
        if n_slots + len(rules) <= 37:
            for r in rules:
                _relist(w, rng, r, 0, N)
            jobs.add(j)
            n_slots += len(rules)
    w.add_job([([], [], [], 0)])  # slot R: a gap no patch names
    jobs.add(w.add_job([([0, N - 1], [info["g_top"]], [N - 2], 0), ([5 % N], [], [], 0), ([N - 1], [], [], 1)]))
    slots, m1 = p.patch(jobs)
    assert len(slots) == 40 and slots.max() == R + 3 and R not in slots
    p.check(m1, due, "patch 1, the wake before it")
    p.check(m1, p.wake(dense=True), "patch 1, dense")
    # 2. more nodes, named only by the patch
    w.n_nodes = Nn
    jobs = set()
    for j in rng.choice(_job_of(w, info["first"]), 6, replace=False):
        for r in w.rules_of(j):
            _relist(w, rng, r, N - 20, Nn)
            w.nids[r] = np.append(w.nids[r], rng.integers(N, Nn)).astype(np.int32)
        jobs.add(j)
    w.nids[info["many"]] = np.append(w.nids[info["many"]], [Nn - 1, N, N]).astype(np.int32)
    jobs.add(_job_of(w, info["many"]))
    slots, m2 = p.patch(jobs)
    assert len(m2[2]) == Nn + 1 and m2[2][Nn] > m2[2][N] and m2[2][Nn] > m2[2][Nn - 1]
    due = list(range(p.n))
    p.check(m2, due, "patch 2, the dense wake before it")
    p.check(m2, p.wake(dense=False), "patch 2, sparse")
    p.check(m2, p.wake(dense=True), "patch 2, dense")
    check_ranges(p.d, [0, N - 1, N, Nn - 1])
    p.d.free()


def test_patch_at_the_top_nodes_only(eng):
    """65537 nodes, a patch whose removed and new pairs all sit on nodes >=
    65000: the survivor tiles in front of them move by one uniform shift, the
    ones among and behind them search."""
    N, lo = 65537, 65000
    key, rin, info = case(N, 2)
    rng = np.random.default_rng(8)
    w0 = World(rin)
    single = [j for j in range(_job_of(w0, info["first"])) if len(w0.rules_of(j)) == 1 and not w0.job_pause[j]]
    jobs = single[3:23]
    for j in jobs:
        (r,) = w0.rules_of(j)
        w0.nids[r], w0.gids[r] = rng.integers(lo, N, 40).astype(np.int32), np.zeros(0, np.int32)
        w0.ex[r] = np.zeros(0, np.int32)
    p = Patched(eng, w0.pack(), CUMULATIVE, extra_slots=0)
    before = JM.join(p.rin, CUMULATIVE)
    due = p.wake(dense=True)
    p.check(before, due, "bound")
    for j in jobs[::2]:
        (r,) = p.w.rules_of(j)
        p.w.nids[r] = rng.integers(lo, N, 25).astype(np.int32)
    _, m = p.patch(jobs[::2])
    assert np.array_equal(m[2][:lo + 1], before[2][:lo + 1]) and not np.array_equal(m[3], before[3])
    assert before[2][lo] > 64 * 2048  # dozens of tiles in front
    p.check(m, due, "patched")
    p.d.free()


# ------------------------------------------------------------------ g. profile

def test_profile_per_node_at_three_passes(eng):
    """Two 30-minute buckets of `@every 30m`: every rule fires once in each, so
    a node's count in a bucket is its degree in the join."""
    key, rin, _ = case(65537, 2)
    m = model(key, rin, CUMULATIVE)
    sp = eng.upload([EVERY30M] * rin.n_rules)
    dr = eng.upload_rules(rin)
    nodes = eng.profile_per_node(sp, None, T0, 1800, 2, dr, CUMULATIVE)
    deg = np.diff(m[2])
    assert nodes.shape == (65537, 2)
    assert np.array_equal(nodes[:, 0], deg) and np.array_equal(nodes[:, 1], deg)
    assert nodes.sum(axis=0).tolist() == [len(m[3])] * 2
    assert eng.profile_totals().tolist() == [rin.n_rules] * 2
    for x in (sp, dr):
        x.free()
