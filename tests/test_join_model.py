"""The host model of the rule -> node join (join_model.py) pinned to the
oracle: O.node_rules over every node for the transpose, or_rule_on_node row by
row for the rule-major CSR, at the node counts the oracle can walk.  The GPU
tests (test_gpu_join.py) hold the kernels to this model at the node counts the
oracle cannot reach."""
import ctypes as C

import numpy as np
import pytest

import join_model as JM
import oracle_lib as O
from cronsun_amd import synth
from cronsun_amd.engine import RulesIn
from join_cases import EDGE_RULES, edge_rules, nid_rules
from patch_common import World

MODES = (JM.EXCLUDE_NONE, JM.EXCLUDE_RULE, JM.EXCLUDE_CUMULATIVE)


def oracle_rows(rin, mode, rules):
    """or_rule_on_node over every node for each of `rules`."""
    js = O.jobset(rin)
    on = O.lib().or_rule_on_node
    return [np.array([n for n in range(rin.n_nodes) if on(C.byref(js), mode, r, n)], dtype=np.int32)
            for r in rules]


def check_vs_oracle(rin, mode, rules):
    rn_off, rn_nodes, nt_off, nt_rule = JM.join(rin, mode)
    assert rn_off.dtype == np.int64 and nt_off.dtype == np.int64
    assert rn_nodes.dtype == np.int32 and nt_rule.dtype == np.int32
    off, rls = O.node_rules(rin, mode, np.arange(rin.n_nodes, dtype=np.int32))
    assert np.array_equal(nt_off, off) and np.array_equal(nt_rule, rls)
    assert len(rn_off) == rin.n_rules + 1 and rn_off[0] == 0 and rn_off[-1] == len(rn_nodes) == len(nt_rule)
    for r, row in zip(rules, oracle_rows(rin, mode, rules)):
        assert np.array_equal(rn_nodes[rn_off[r]:rn_off[r + 1]], row), r
    return rn_off, rn_nodes, nt_off, nt_rule


@pytest.mark.parametrize("per", [(1, 4), (6, 12)])
@pytest.mark.parametrize("keys", [0, 1, 2, 3])
@pytest.mark.parametrize("N", [1, 33, 64, 65, 257, 2049])
def test_model_vs_oracle(N, keys, per):
    """Every set holds paused jobs, missing groups named by rules, repeated
    NodeIDs, excludes >= N, rules without nodes, the all-nodes group and a
    group of more than 64 members (edge_rules)."""
    R = 60 + EDGE_RULES
    rin, info = edge_rules(N, R, keys, seed=100 + N + keys, rules_per_job=per)
    assert rin.job_pause.any() and not rin.group_exists[:rin.n_groups].all()
    gids = rin.gids[:rin.gid_off[R]]
    assert (rin.group_exists[gids] == 0).any()
    assert (rin.ex[:rin.ex_off[R]] >= N).any()
    sizes = np.diff(rin.group_off[:rin.n_groups + 1])
    assert sizes[info["g_all"]] == N and (sizes > 64).any()
    many = rin.nids[rin.nid_off[info["many"]]:rin.nid_off[info["many"] + 1]]
    assert len(many) == 130 and len(np.unique(many)) < 130
    # rows by or_rule_on_node: all of them up to 65 nodes, above that the
    # planted rules and every seventh synthetic one
    rules = range(R) if N <= 65 else sorted(set(range(info["first"], R)) | set(range(0, R, 7)))
    for mode in MODES:
        rn_off, rn_nodes, nt_off, _ = check_vs_oracle(rin, mode, rules)
        deg = np.diff(rn_off)
        assert deg[list(info["paused"])].sum() == 0 and deg[list(info["empty"])].sum() == 0
        assert nt_off[1] > nt_off[0] and nt_off[N] > nt_off[N - 1]  # nodes 0 and N-1 run something
        if keys != 1:
            assert deg[list(info["all_nodes"])].max() >= N - 2
    # a GroupID past the group table or negative is skipped like a missing one
    rin.gids[:rin.gid_off[R]][::5] = rin.n_groups + 3
    rin.gids[:rin.gid_off[R]][1::5] = -1
    for mode in MODES:
        check_vs_oracle(rin, mode, range(0, R, 3))


def _hand():
    """6 rules x 5 nodes.  Job 0: rules 0-2, one key; job 1: rules 3 (key 7)
    and 4 (key 8); job 2: rule 5, paused.  Groups: 0 = {1, 2}, 1 = {0, 4},
    2 = {3} missing."""
    nids = [[0, 1, 2, 3], [1, 2, 3], [2, 4], [3, 3], [], [0, 1]]
    gids = [[], [], [2], [0], [1], []]
    ex = [[1], [3], [], [9, 4], [], []]
    groups = [[1, 2], [0, 4], [3]]

    def csr(lists):
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        return off, np.array([v for x in lists for v in x], dtype=np.int32)
    nid_off, nid = csr(nids)
    gid_off, gid = csr(gids)
    ex_off, exv = csr(ex)
    group_off, group_nodes = csr(groups)
    return RulesIn(5, 3, 6, 3, rule_key=[7, 7, 7, 7, 8, 7], group_off=group_off, group_nodes=group_nodes,
                   group_exists=[1, 1, 0], rule_job=[0, 0, 0, 1, 1, 2], nid_off=nid_off, nids=nid,
                   gid_off=gid_off, gids=gid, ex_off=ex_off, ex=exv, job_pause=[0, 0, 1])


# Sets before shadowing (rule: NONE / RULE / CUMULATIVE):
#   0: 0123 / 023 / 023    1: 123 / 12 / 2     2: 24 / 24 / 24
#   3: 123 / 123 / 123     4: 04 / 04 / 0 (job 1's excludes so far: 9, 4)    5: paused
# Shadowing inside job 0 (one key): rule 0 loses what rules 1 and 2 hold, rule 1
# what rule 2 holds.  Rule 1 excludes node 3, so under RULE and CUMULATIVE it does
# not shadow rule 0 there and rule 0 keeps node 3; under NONE it does.
HAND = {
    JM.EXCLUDE_NONE: ([0, 1, 3, 5, 8, 10, 10], [0, 1, 3, 2, 4, 1, 2, 3, 0, 4],
                      [0, 2, 4, 6, 8, 10], [0, 4, 1, 3, 2, 3, 1, 3, 2, 4]),
    JM.EXCLUDE_RULE: ([0, 2, 3, 5, 8, 10, 10], [0, 3, 1, 2, 4, 1, 2, 3, 0, 4],
                      [0, 2, 4, 6, 8, 10], [0, 4, 1, 3, 2, 3, 0, 3, 2, 4]),
    JM.EXCLUDE_CUMULATIVE: ([0, 2, 2, 4, 7, 8, 8], [0, 3, 2, 4, 1, 2, 3, 0],
                            [0, 2, 3, 5, 7, 8], [0, 4, 3, 2, 3, 0, 3, 2]),
}


@pytest.mark.parametrize("mode", MODES)
def test_hand_worked(mode):
    rin = _hand()
    got = check_vs_oracle(rin, mode, range(6))
    for g, e in zip(got, HAND[mode]):
        assert g.tolist() == e


def test_degenerate_sets():
    for rin in (nid_rules(5, []), nid_rules(4, [[0, 1], [3]], pause=[1, 1]), nid_rules(1, [[0], [0, 0]])):
        for mode in MODES:
            rn_off, rn_nodes, nt_off, nt_rule = check_vs_oracle(rin, mode, range(rin.n_rules))
            assert len(nt_off) == rin.n_nodes + 1
    with pytest.raises(ValueError):
        JM.join(nid_rules(5, []), 3)


def test_due_filter_brute_force():
    rng = np.random.default_rng(3)
    rin, _ = edge_rules(33, 80, 2, seed=9)
    _, _, nt_off, nt_rule = JM.join(rin, JM.EXCLUDE_RULE)
    for due in ([], [5], list(range(80)), [79, 3, 200], rng.choice(90, 40, replace=False).tolist()):
        off, slots = JM.due_filter(nt_off, nt_rule, due)
        exp_off, exp = [0], []
        for n in range(33):
            exp += [int(r) for r in nt_rule[nt_off[n]:nt_off[n + 1]] if int(r) in due]
            exp_off.append(len(exp))
        assert off.tolist() == exp_off and slots.tolist() == exp
        assert off.dtype == np.int64 and slots.dtype == np.int32
    off, slots = JM.due_filter(np.zeros(4, np.int64), np.zeros(0, np.int32), [1, 2])
    assert off.tolist() == [0, 0, 0, 0] and len(slots) == 0


@pytest.mark.parametrize("keys", [0, 2])
def test_patched_brute_force(keys):
    """patched(rin, patch, slots) joins to what the edited World packs to:
    replaced and emptied rows, a flipped pause, slots past R with a gap, more
    nodes."""
    rin = synth.multi_rule_jobs(30, n_nodes=20, seed=4, key_choices=keys)
    w = World(rin)
    R, N = w.n_rules, w.n_nodes
    w.n_nodes = N + 7
    for r in w.rules_of(3) + w.rules_of(11):
        w.nids[r] = np.array([1, N + 6, 5, N], np.int32)
        w.ex[r] = np.array([5], np.int32)
    for r in w.rules_of(8):
        w.nids[r], w.gids[r] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    w.job_pause[5] ^= 1
    gap = w.add_job([([], [], [], 0)])  # slot R: set in the dispatcher, named by no patch
    new = [w.add_job([([N + 1, 2], [0], [], 0), ([N + 1, 3], [], [2], 0)]), w.add_job([([0], [1], [], 1)])]
    prin, slots = w.patch([3, 11, 8, 5] + new)
    assert slots.max() == R + 3 and R not in slots and gap == rin.n_jobs
    got = JM.patched(rin, prin, slots)
    full = w.pack()
    assert (got.n_nodes, got.n_rules, got.n_groups) == (N + 7, R + 4, full.n_groups)
    for mode in MODES:
        a, b = JM.join(got, mode), JM.join(full, mode)
        assert b[0][-1] > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
        off, rls = O.node_rules(full, mode, np.arange(full.n_nodes, dtype=np.int32))
        assert np.array_equal(a[2], off) and np.array_equal(a[3], rls)
    # the untouched set: patched with nothing is the set itself
    same = JM.patched(rin, rin.slice_rules(0, 0), [])
    assert all(np.array_equal(x, y) for x, y in zip(JM.join(same, 2), JM.join(rin, 2)))
