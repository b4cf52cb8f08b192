"""The host model of the fire profile (profile_model.py) pinned on the CPU: its
two node-matrix forms against each other, its node matrix over the join model
against the oracle's join on the rule sets of test_gpu_profile.py, its totals
against a column sum, bin_fires against oracle_profile, one case by hand, and
the properties of make_pick and the base sets that the GPU tests
(test_gpu_profile_scale.py) rely on."""
import numpy as np
import pytest

import join_model as JM
import profile_cases as PC
import profile_model as PM

MODES = (JM.EXCLUDE_NONE, JM.EXCLUDE_RULE, JM.EXCLUDE_CUMULATIVE)


def random_join(rng, N, R, density, full_node=None, empty_nodes=(), empty_rules=()):
    """A node-major join drawn pair by pair: (nt_off, nt_rule)."""
    on = rng.random((N, R)) < density
    if full_node is not None:
        on[full_node] = True
    on[list(empty_nodes)] = False
    on[:, list(empty_rules)] = False
    if full_node is not None and len(empty_rules) == 0:
        assert on[full_node].all()
    node, rule = np.nonzero(on)  # node-major, rules ascending
    nt_off = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N))]).astype(np.int64)
    return nt_off, rule.astype(np.int32)


@pytest.mark.parametrize("K,N,R,B", [(1, 5, 40, 3), (7, 1, 30, 1), (13, 40, 500, 65), (50, 9, 2000, 130)])
def test_node_matrix_two_ways(K, N, R, B):
    """Segment sums over base[pick] against W @ base: empty nodes (the first,
    the last, two neighbours), rules on no node, a node holding every rule,
    K = 1, N = 1."""
    rng = np.random.default_rng(K * 1000 + N)
    base = rng.integers(0, 61, (K, B)).astype(np.int32)
    base[rng.random(K) < 0.2] = 0
    pick = PM.make_pick(K, R, seed=R)
    for full, empty_nodes, empty_rules in ((None, (), ()), (N // 2, (0, N - 1) if N > 2 else (), (3, R - 1)),
                                           (N - 1, (1, 2) if N > 3 else (), ()), (None, range(N), ())):
        nt_off, nt_rule = random_join(rng, N, R, 0.3, full, empty_nodes, empty_rules)
        a = PM.node_matrix(nt_off, nt_rule, PM.rule_matrix(base, pick))
        b = PM.node_matrix_tiled(nt_off, nt_rule, pick, base)
        assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (N, B)
        assert np.array_equal(a, b)
        for n in empty_nodes:
            assert not a[n].any()
        if full is not None and len(empty_rules) == 0:
            assert np.array_equal(a[full], PM.totals(base, pick))
        # and the plain loop
        for n in range(0, N, max(1, N // 5)):
            rows = base[pick[nt_rule[nt_off[n]:nt_off[n + 1]]]]
            assert np.array_equal(a[n], rows.sum(axis=0, dtype=np.int64))


def test_node_matrix_does_not_wrap_int32():
    """70 000 rules of 40 000 fires in a bucket on one node: 2.8e9."""
    base = np.array([[40000, 1]], dtype=np.int32)
    pick = np.zeros(70000, dtype=np.int64)
    nt_off, nt_rule = np.array([0, 70000], dtype=np.int64), np.arange(70000, dtype=np.int32)
    exp = [[2_800_000_000, 70000]]
    assert PM.node_matrix(nt_off, nt_rule, base[pick]).tolist() == exp
    assert PM.node_matrix_tiled(nt_off, nt_rule, pick, base).tolist() == exp
    assert PM.totals(base, pick).tolist() == exp[0]


@pytest.mark.parametrize("name", ["nodes48", "keys3"])
def test_node_matrix_vs_oracle_join(name):
    """node_matrix over JM.join equals the oracle's per-node filter applied to
    the oracle's rule matrix, in the three exclude modes, on the two rule sets
    of test_gpu_profile.py (a node every rule names, a node no rule reaches,
    paused jobs, repeated Cmd keys)."""
    rin, _, oscheds = PC.rule_set(name)
    w, B = 60, 65
    rules = PC.oracle_profile(oscheds, "UTC", PC.T0_UTC, w, B)
    seen = []
    for mode in MODES:
        _, _, nt_off, nt_rule = JM.join(rin, mode)
        exp, roff = PC.oracle_node_matrix(rin, mode, rules)
        assert np.array_equal(nt_off, roff)
        got = PM.node_matrix(nt_off, nt_rule, rules)
        assert np.array_equal(got, exp)
        assert got[rin.n_nodes - 2].any() and not got[rin.n_nodes - 1].any()
        seen.append(got)
    assert not np.array_equal(seen[0], seen[2])


def test_totals_is_the_column_sum():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 3601, (37, 130)).astype(np.int32)
    for R in (1, 36, 37, 5000):
        pick = PM.make_pick(37, R, seed=R)
        got = PM.totals(base, pick)
        assert got.dtype == np.int64
        assert np.array_equal(got, base[pick].sum(axis=0, dtype=np.int64))


@pytest.mark.parametrize("w,B", [(60, 65), (7, 1000)])
def test_bin_fires_vs_oracle_profile(w, B):
    """The base set's one expansion over its longest horizon, binned, equals
    oracle_profile's own expansion to t0 + w * B."""
    base = PC.utc_base()
    exp = PC.oracle_profile(PC.oracle_parse_all(base.specs), "UTC", base.t0, w, B)
    got = base.matrix(w, B)
    assert got.dtype == np.int32 and np.array_equal(got, exp)
    assert got.sum() < len(base.times)  # fires past w * B were dropped


def test_by_hand():
    """Three rules, two nodes, two buckets of 10 s from t0 = 100.
    Fires: rule 0 at 101, 110, 111; rule 1 at 120; rule 2 none.
    Bucket 0 = (100, 110], bucket 1 = (110, 120].
    Node 0 runs rules 0 and 1, node 1 runs rules 1 and 2."""
    off = np.array([0, 3, 4, 4], dtype=np.int64)
    times = np.array([101, 110, 111, 120], dtype=np.int64)
    base = PM.bin_fires(off, times, 100, 10, 2)
    assert base.tolist() == [[2, 1], [0, 1], [0, 0]]
    assert PM.bin_fires(off, times, 100, 10, 1).tolist() == [[2], [0], [0]]  # 111 and 120 dropped
    assert PM.bin_fires(off, times, 100, 5, 4).tolist() == [[1, 1, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]
    pick = np.arange(3)
    assert PM.totals(base, pick).tolist() == [2, 2]
    nt_off, nt_rule = np.array([0, 2, 4], dtype=np.int64), np.array([0, 1, 1, 2], dtype=np.int32)
    assert PM.node_matrix(nt_off, nt_rule, base).tolist() == [[2, 2], [0, 1]]
    assert PM.node_matrix_tiled(nt_off, nt_rule, pick, base).tolist() == [[2, 2], [0, 1]]
    # rule r = base rule pick[r]: five rules 0 2 0 1 0, node 0 runs 0, 2, 4, node 1 runs 3
    pick = np.array([0, 2, 0, 1, 0])
    assert PM.rule_matrix(base, pick).tolist() == [[2, 1], [0, 0], [2, 1], [0, 1], [2, 1]]
    assert PM.totals(base, pick).tolist() == [6, 4]
    nt_off, nt_rule = np.array([0, 3, 4], dtype=np.int64), np.array([0, 2, 4, 3], dtype=np.int32)
    assert PM.node_matrix_tiled(nt_off, nt_rule, pick, base).tolist() == [[6, 3], [0, 1]]
    assert PM.node_weights(nt_off, nt_rule, pick, 3).tolist() == [[3, 0, 0], [0, 1, 0]]


@pytest.mark.parametrize("K,R", [(2, 50), (3, 6), (202, 4095), (600, 1025), (600, 4095), (600, 1 << 20)])
def test_make_pick(K, R):
    pick = PM.make_pick(K, R, seed=K + R)
    assert pick.shape == (R,) and pick.min() >= 0 and pick.max() < K
    assert (pick[1:] != pick[:-1]).all()
    if 2 * R >= 3 * K:
        assert len(np.unique(pick)) == K


def test_base_sets_hold_what_the_gpu_tests_need():
    """The UTC base: at most three every-second rules, a seconds table, @every
    delays that divide none of the widths used (7 s, 90 min, 100 h against 13,
    20, 60, 3600), rules that never fire, and at least half of its rows
    pairwise distinct over its horizon.  The zone base: a rule with fires on
    both sides of the transition."""
    b = PC.utc_base()
    assert 590 <= b.K <= 610
    assert 1 <= b.specs.count("* * * * * *") <= 3
    assert all(s in b.specs for s in PC.EXTRA)
    fine = b.matrix(20, 4096)
    fires = fine.sum(axis=1)
    assert fires[b.specs.index("0 0 0 30 Feb ?")] == 0 and fires[b.specs.index("@every 100h")] == 0
    assert fires[b.specs.index("* * * * * *")] == 20 * 4096
    assert 2 * len(np.unique(fine, axis=0)) >= b.K
    z = PC.zone_base()
    assert 195 <= z.K <= 202
    m = z.matrix(1800, 24)
    assert (m[:, :12].sum(axis=1) > 0).sum() > 20 and (m[:, 12:].sum(axis=1) > 0).sum() > 20
