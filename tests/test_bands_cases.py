"""The cases of tests/bands_cases.py hold what they promise, and its numpy
model of the per-node CSR equals the oracle's with no shortcut through the
kinds: O.node_rules membership, O.expand_batch of every rule, O.node_list.
They keep tests/test_gpu_pernode_bands.py from passing because a case lost its
point."""
import numpy as np
import pytest

import bands_cases as BC
import oracle_lib as O
from common import oracle_zone

B = BC.B
I32 = 1 << 31


def oracle_csr(case, nodes):
    """the oracle's lists of `nodes`, concatenated: (off [len(nodes)+1], time, rule)"""
    rin = BC.rules_in(case)
    if len(nodes) <= 64:  # each node's own filter over every rule
        roff, rules = O.node_rules(rin, 0, nodes)
    else:  # every node: or_rule_on_node over each rule's listed nodes, transposed
        assert np.array_equal(nodes, np.arange(case.n_nodes))
        js, L = O.jobset(rin), O.lib()
        pr, pn = [], []
        for r in range(rin.n_rules):
            for n in rin.nids[rin.nid_off[r]:rin.nid_off[r + 1]].tolist():
                if L.or_rule_on_node(js, 0, r, n):
                    pr.append(r)
                    pn.append(n)
        pr, pn = np.array(pr, np.int64), np.array(pn, np.int64)
        o = np.argsort(pn, kind="stable")
        rules, roff = pr[o], np.searchsorted(pn[o], np.arange(case.n_nodes + 1))
        some = np.sort(np.random.default_rng(3).choice(case.n_nodes, 48, replace=False))
        soff, srules = O.node_rules(rin, 0, some)
        for i, n in enumerate(some.tolist()):
            assert np.array_equal(srules[soff[i]:soff[i + 1]], rules[roff[n]:roff[n + 1]]), n
    rules = rules.astype(np.int64)
    if len(nodes) * 4 > case.n_nodes:  # every rule once
        eo, et = O.expand_batch(BC.oracle_schedules(case, np.arange(BC.n_rules(case))), case.t0, case.t1,
                                oracle_zone(case.zone))
        time, rule = O.node_list(eo, et, rules)
    else:  # the rules of these nodes, one schedule per (node, rule)
        eo, et = O.expand_batch(BC.oracle_schedules(case, rules), case.t0, case.t1, oracle_zone(case.zone))
        time, pos = O.node_list(eo, et, np.arange(len(rules)))
        return eo[roff], time, rules[pos].astype(np.int32)
    lens = np.concatenate([[0], np.cumsum(eo[rules + 1] - eo[rules])])
    return lens[roff], time, rule


def check_shape(case):
    R = BC.n_rules(case)
    assert case.K == -(-R // B)
    per = BC.fires_per_rule(case)
    assert per >= 6, per
    E = int(round(per * R))
    assert E < 1 << 30 and BC.band_rules(R, E) == B
    return BC.segments(case)


@pytest.mark.parametrize("name", BC.SMALL)
def test_model_equals_oracle_every_node(name):
    case = BC.CASES[name]()
    off, time, rule = BC.expected(case)
    assert off.dtype == np.int64 and time.dtype == np.int64 and rule.dtype == np.int32
    o_off, o_time, o_rule = oracle_csr(case, np.arange(case.n_nodes))
    assert np.array_equal(off, o_off)
    assert np.array_equal(time, o_time) and np.array_equal(rule, o_rule)
    if name != "overflow3":  # (3 days: no time-order test runs it)
        check_time_order(case, (off, time, rule), np.arange(min(case.n_nodes, 40)))


@pytest.mark.parametrize("name", BC.LARGE)
def test_model_equals_oracle_sampled_nodes(name):
    case = BC.CASES[name]()
    off, time, rule = BC.expected(case)
    nodes = np.sort(np.random.default_rng(5).choice(case.n_nodes, 2 if case.n_nodes <= 5 else 6, replace=False))
    o_off, o_time, o_rule = oracle_csr(case, nodes)
    for i, n in enumerate(nodes.tolist()):
        a, b = int(off[n]), int(off[n + 1])
        assert b - a == o_off[i + 1] - o_off[i] > 0, n
        assert np.array_equal(time[a:b], o_time[o_off[i]:o_off[i + 1]]), n
        assert np.array_equal(rule[a:b], o_rule[o_off[i]:o_off[i + 1]]), n
    check_time_order(case, (off, time, rule), nodes)


def check_time_order(case, csr, nodes):
    """by_time against a plain lexsort by (time, rule) of each node's list"""
    off, time, rule = csr
    off2, time2, rule2 = BC.by_time(case, csr, case.t0)
    assert off2 is off and len(time2) == len(time)
    for n in np.asarray(nodes).tolist():
        a, b = int(off[n]), int(off[n + 1])
        o = np.lexsort((rule[a:b], time[a:b]))
        assert np.array_equal(time2[a:b], time[a:b][o]) and np.array_equal(rule2[a:b], rule[a:b][o]), n


def test_edges3_properties():
    case = BC.edges3()
    seg = check_shape(case)
    R = BC.n_rules(case)
    assert R == 2 * B + 1 and case.K == 3 and case.n_nodes == 7
    pnode, prule = BC.pairs("edges3")
    assert prule[pnode == 0].tolist() == [B - 1, B, B + 1, 2 * B - 1, 2 * B]
    # node 0: both band boundaries of its list inside its first 64-event block
    assert seg.start[0, 0] == 0 and (seg.events[0] > 0).all()
    assert 0 < seg.start[0, 1] < seg.start[0, 2] < 64 < seg.start[0, 2] + seg.events[0, 2]
    assert seg.events[1].tolist()[::2] == [0, 0] and seg.events[1, 1] > 0 and prule[pnode == 1][0] == B
    assert seg.events[2, 1] == 0 and seg.events[2, 0] > 0 and seg.events[2, 2] > 0
    assert seg.pairs[3].sum() == 0
    # node 4: several rounds of 256 pairs per segment, ragged event counts
    assert (seg.pairs[4, :2] > 4 * 256).all() and (seg.events[4, :2] % 64 != 0).all()
    assert (seg.start[4, :2] % 64 != 0).all()
    assert seg.pairs[5].tolist() == [0, 0, 1] and seg.events[5, 2] == 600
    assert prule[pnode == 6].tolist() == [0, R - 1] and (seg.events[6, ::2] > 0).all()
    # the first rule of band 1 is gathered, the first of band 2 a progression
    x, prog = BC.record_x(case)
    assert not prog[prule == B].any() and prog[prule == 2 * B].all()
    assert case.kinds[case.kind[B]] == BC.GATHERED and case.kinds[case.kind[2 * B]] == BC.SECOND
    # never-firing rules, progressions and the non-progression, in every band of node 4
    for k in range(2):
        kinds4 = {case.kinds[i] for i in case.kind[prule[(pnode == 4) & (prule // B == k)]]}
        assert kinds4 >= {BC.NEVER, "*/10 * * * * *", "@every 7s", "0 * * * * *", BC.GATHERED}
    # the short window of the band-width test: fewer than 6 fires per rule, wider bands
    per = BC.fires_per_rule(case, case.t0, case.t0 + BC.EDGES3_SHORT)
    assert 0 < per < 6 and BC.band_rules(R, int(round(per * R))) == 2 * B


def test_many_nodes3_properties():
    case = BC.many_nodes3()
    seg = check_shape(case)
    assert BC.n_rules(case) == 2 * B + 1 and case.K == 3
    assert case.n_nodes * case.K > 131072
    per_node = seg.pairs.sum(1)
    assert (per_node <= 4).all()  # tiny nodes: most segments hold no pair, or pairs that never fire
    assert (seg.pairs == 0).sum() > case.n_nodes and (seg.events == 0).sum() > (seg.pairs == 0).sum() + 1000
    # lists that cross a band boundary
    assert ((seg.events > 0).sum(1) >= 2).sum() > 1000
    assert 4_000_000 < seg.events.sum() < 6_000_000


def test_overflow3_properties():
    case = BC.overflow3()
    seg = check_shape(case)
    assert BC.n_rules(case) == 2 * B + 1 and case.K == 3 and case.t1 - case.t0 == 3 * BC.DAY
    assert seg.events.sum() < 16_000_000
    pnode, prule = BC.pairs("overflow3")
    x, prog = BC.record_x(case)
    fits = (x >= -I32) & (x < I32)
    for k in range(2):  # progression records past int32 (gathered instead) and within it, in bands 0 and 1
        band = prog & (prule // B == k)
        assert (band & ~fits).sum() > 1000 and (band & fits).sum() > 1000, k
    # an every-second rule first in a segment of every band
    sec = case.kinds.index(BC.SECOND)
    first = np.concatenate([[True], (pnode[1:] != pnode[:-1]) | (prule[1:] // B != prule[:-1] // B)])
    assert {int(r) // B for r in prule[first & (case.kind[prule] == sec)]} == {0, 1, 2}


@pytest.mark.parametrize("name", BC.LARGE)
def test_xcd35_properties(name):
    case = BC.CASES[name]()
    seg = check_shape(case)
    R = BC.n_rules(case)
    assert R == (1 << 20) + 2 * B + 77 and case.K == 35
    assert case.K >= 32 and case.K % 8 != 0  # 8 band groups, uneven
    assert R > 1 << 20 and (1 << 20) % B == 0  # the packed time order cuts its tiles at band 32
    # every band of every node holds events (the last one, of 77 rules, on some nodes)
    assert (seg.events[:, :-1] > 0).all() and (seg.events[:, -1] > 0).any() and (seg.events % 64 != 0).any()
    if name == "xcd35_many":
        assert case.n_nodes * case.K > 131072
    assert seg.events.sum() < 20_000_000
