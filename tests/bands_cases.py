"""Constructed rule sets for the per-node path at more than one rule band
(cg_pernode.hip: k_seg_bounds, k_rule_info, k_seg_records, k_node_write; the
tile cuts of cg_node_order.hip), with a numpy model of the whole per-node CSR.
A helper module, not a test: tests/test_bands_cases.py checks the cases and
the model on the CPU, tests/test_gpu_pernode_bands.py runs them on the GPU.

The per-node path cuts every node's list into (node, rule band) segments of B
rules, K = ceil(R / B) bands.  band_rules() keeps B at its floor of 32768 rules
exactly when 1.5 MiB / (8 * E / R) <= 32768, E the window's rule-major fires:
at E / R >= 6.  Every case here says so about itself (fires_per_rule), and the
GPU tests assert (B, K) through cg_node_result_bands.

A case's rules are drawn from a short list of kinds (rule i = kinds[kind[i]]),
membership is explicit (nid_off / nids: no groups, no excludes; the join is not
under test here).  The model asks the oracle for the fires of the distinct
kinds only and assembles every node's list in numpy from the pairs sorted by
(node, rule); the time order is a stable sort by time within each node.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
from common import oracle_parse_all, oracle_zone
from cronsun_amd import synth

DAY = 86400
B = 32768  # CG_BAND_MIN_RULES (cg_pernode.hip)
T0 = synth.T0_2026 + 20 * DAY + 123  # Sunday 2026-01-25 00:02:03 UTC: the yearly rule never fires

NEVER = "0 0 0 1 1 *"
SECOND = "* * * * * *"
GATHERED = "7,30,45 * * * * *"  # no arithmetic progression: the writer gathers its fires
EDGE_KINDS = (NEVER, "*/10 * * * * *", "@every 7s", "0 * * * * *", GATHERED, SECOND)
SPARSE_KINDS = ("0 0 * * * *", "@every 90m", "0 30 9 * * *", "0 0 12 * * 1", NEVER, "0 7,30,45 * * * *", SECOND)
XCD_KINDS = (NEVER, "*/10 * * * * *", "0 * * * * *", "*/30 * * * * *", GATHERED, "@every 7s")

# kind[i] indexes kinds; nid_off / nids: the nodes of every rule, ascending
Case = namedtuple("Case", "name kinds kind n_nodes nid_off nids zone t0 t1 K")


def n_rules(case):
    return len(case.kind)


# ------------------------------------------------------------- membership
def two_nodes_per_rule(R, N):
    """rule i on nodes i % N and (7i + 1) % N (once where they coincide)"""
    i = np.arange(R, dtype=np.int64)
    nd = np.sort(np.stack([i % N, (7 * i + 1) % N], 1), 1)
    same = nd[:, 0] == nd[:, 1]
    nid_off = np.zeros(R + 1, np.int64)
    nid_off[1:] = np.cumsum(np.where(same, 1, 2))
    keep = np.ones((R, 2), bool)
    keep[:, 1] = ~same
    return nid_off, nd[keep].astype(np.int32)


def nodes_of_rules(R, per_node):
    """per_node[n] = the rules of node n -> (nid_off, nids)"""
    rule = np.concatenate([np.asarray(r, np.int64) for r in per_node])
    node = np.concatenate([np.full(len(r), n, np.int64) for n, r in enumerate(per_node)])
    o = np.lexsort((node, rule))
    nid_off = np.zeros(R + 1, np.int64)
    nid_off[1:] = np.cumsum(np.bincount(rule, minlength=R))
    return nid_off, node[o].astype(np.int32)


def rules_in(case):
    """the case's membership as the product's RulesIn (one job per rule)"""
    from cronsun_amd.engine import RulesIn
    R = n_rules(case)
    z = np.zeros(R + 1, np.int64)
    return RulesIn(case.n_nodes, 0, R, R, group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.arange(R, dtype=np.int32), nid_off=case.nid_off,
                   nids=case.nids, gid_off=z, gids=np.zeros(0, np.int32), ex_off=z, ex=np.zeros(0, np.int32),
                   job_pause=np.zeros(R, np.uint8))


def schedules(case):
    """the product's cg_schedule array of the case: the kinds parsed once, indexed by kind"""
    from cronsun_amd import cron
    karr, status = cron.parse_batch(list(case.kinds), threads=1)
    assert not np.any(status)
    a = np.ascontiguousarray(np.ctypeslib.as_array(karr)[case.kind])
    arr = (karr._type_ * n_rules(case)).from_buffer(a)
    return arr


def oracle_schedules(case, rules):
    """the oracle's schedule of each of `rules`, one entry per rule"""
    karr = O.sched_array(oracle_parse_all(case.kinds))
    rows = np.frombuffer(karr, np.uint8).reshape(len(case.kinds), -1)  # one OrSched per row
    a = np.ascontiguousarray(rows[case.kind[np.asarray(rules, np.int64)]])
    return (O.OrSched * len(a)).from_buffer(a)


# ------------------------------------------------------------------ cases
def _uniform_kinds(R, n_kinds, seed):
    return np.random.default_rng(seed).integers(0, n_kinds, R).astype(np.int64)


def _edge_kinds(R):
    """uniformly the first five EDGE_KINDS; the rules at the band edges fixed:
    B (first of band 1) gathered, 2B (first and only rule of band 2) every second"""
    k = {s: i for i, s in enumerate(EDGE_KINDS)}
    kind = _uniform_kinds(R, 5, 7)
    kind[0] = k["*/10 * * * * *"]
    kind[B - 1] = kind[B + 1] = kind[2 * B - 1] = k["0 * * * * *"]
    kind[B] = k[GATHERED]
    kind[2 * B] = k[SECOND]
    return kind


@functools.lru_cache(maxsize=None)
def edges3():
    """R = 2B + 1, K = 3 (the last band is rule 2B alone), 7 nodes, 600 s:
      0  rules B-1, B, B+1, 2B-1, 2B: 10, 30, 10, 10 and 600 fires, so both
         band boundaries of its list lie in its first 64-event block
      1  every 5th rule of band 1 from rule B: empty first and last segments
      2  every 7th rule of band 0 and rule 2B: an empty middle segment
      3  no rules
      4  every third rule: thousands of pairs per segment
      5  rule 2B alone (every second): one record across many blocks
      6  rules 0 and R-1"""
    R = 2 * B + 1
    per_node = [[B - 1, B, B + 1, 2 * B - 1, 2 * B], np.arange(B, 2 * B, 5),
                np.concatenate([np.arange(3, B, 7), [2 * B]]), [], np.arange(0, R, 3), [2 * B], [0, R - 1]]
    nid_off, nids = nodes_of_rules(R, per_node)
    return Case("edges3", EDGE_KINDS, _edge_kinds(R), 7, nid_off, nids, "UTC", T0, T0 + 600, 3)


EDGES3_SHORT = 60  # s: E / R < 6, so band_rules widens the bands of edges3 to 65536 rules (K = 2)


@functools.lru_cache(maxsize=None)
def many_nodes3():
    """edges3's rules on 50 000 nodes, two per rule: N * K = 150 000 > 131 072
    segments (k_seg_records: runs of per > 1 segments per half-wave, across
    band changes); most nodes hold one to three rules, some none."""
    R, N = 2 * B + 1, 50_000
    nid_off, nids = two_nodes_per_rule(R, N)
    return Case("many_nodes3", EDGE_KINDS, _edge_kinds(R), N, nid_off, nids, "UTC", T0, T0 + 600, 3)


@functools.lru_cache(maxsize=None)
def overflow3():
    """R = 2B + 1, 6 nodes, two per rule, 3 days of sparse rules (hourly,
    @every 90m, daily, weekly, never, three minutes of every hour) with
    every-second rules (259 200 fires) first in their nodes' segments: rules 0
    and 1 (band 0: nodes 0, 1, 2), B and B + 1 (band 1: nodes 2, 3, 4) and 2B
    (band 2).  The positions of the progression rules behind them no longer
    fit the record's 32-bit x (first fire - position * stride), so those fall
    back to gathers."""
    R, N = 2 * B + 1, 6
    kind = _uniform_kinds(R, 6, 11)
    kind[[0, 1, B, B + 1, 2 * B]] = SPARSE_KINDS.index(SECOND)
    kind[[2, B + 2]] = SPARSE_KINDS.index("0 30 9 * * *")  # a daily rule right behind them
    nid_off, nids = two_nodes_per_rule(R, N)
    return Case("overflow3", SPARSE_KINDS, kind, N, nid_off, nids, "UTC", T0, T0 + 3 * DAY, 3)


R_XCD = (1 << 20) + 2 * B + 77  # K = 35: not a multiple of the 8 band groups; past 2^20 rules


@functools.lru_cache(maxsize=None)
def xcd35():
    """K = 35 bands (k_seg_records' 8 band groups, uneven; the packed time
    order's tiles cut at band 32), 5 nodes, two per rule, 120 s."""
    nid_off, nids = two_nodes_per_rule(R_XCD, 5)
    return Case("xcd35", XCD_KINDS, _uniform_kinds(R_XCD, 6, 13), 5, nid_off, nids, "UTC", T0, T0 + 120, 35)


@functools.lru_cache(maxsize=None)
def xcd35_many():
    """xcd35's rules on 4099 nodes: N * K = 143 465 > 131 072 segments, so the
    band groups walk runs of per > 1 segments."""
    nid_off, nids = two_nodes_per_rule(R_XCD, 4099)
    return Case("xcd35_many", XCD_KINDS, _uniform_kinds(R_XCD, 6, 13), 4099, nid_off, nids, "UTC", T0, T0 + 120,
                35)


CASES = {"edges3": edges3, "many_nodes3": many_nodes3, "overflow3": overflow3, "xcd35": xcd35,
         "xcd35_many": xcd35_many}
SMALL = ("edges3", "many_nodes3", "overflow3")  # K = 3
LARGE = ("xcd35", "xcd35_many")


# ------------------------------------------------------------------ model
def band_rules(R, E):
    """cg_pernode.hip band_rules(): rules per band for R rules and E rule-major
    fires (below 2^30 fires; past that the call halves the bands further)"""
    want = int(1536 * 1024 / (max(E, 1) * 8.0 / max(R, 1)))
    p = B
    while p < want and p < R and p < 1 << 20:
        p <<= 1
    return p


def _stable_by(key, n_values):
    """stable argsort of small non-negative keys (numpy's radix sort for 16 bits)"""
    if n_values <= 1 << 16:
        return np.argsort(key.astype(np.uint16), kind="stable")
    return np.argsort(key, kind="stable")


@functools.lru_cache(maxsize=None)
def pairs(name):
    """the case's (node, rule) pairs sorted by (node, rule): (pair_node, pair_rule)"""
    case = CASES[name]()
    rule = np.repeat(np.arange(n_rules(case), dtype=np.int64), np.diff(case.nid_off))
    node = case.nids.astype(np.int64)
    o = _stable_by(node, case.n_nodes)  # rules ascend already
    return node[o], rule[o]


def kind_fires(case, t0, t1):
    """the oracle's fire lists of the distinct kinds over (t0, t1]: CSR (ko, kt)"""
    return O.expand_batch(O.sched_array(oracle_parse_all(case.kinds)), t0, t1, oracle_zone(case.zone))


def fires_per_rule(case, t0=None, t1=None):
    """E / R of the window's rule-major expansion"""
    t0, t1 = (case.t0, case.t1) if t0 is None else (t0, t1)
    ko, _ = kind_fires(case, t0, t1)
    return float(np.diff(ko)[case.kind].sum()) / n_rules(case)


def _pair_counts(case, t0, t1):
    ko, kt = kind_fires(case, t0, t1)
    pnode, prule = pairs(case.name)
    pcnt = np.diff(ko)[case.kind[prule]]
    poff = np.concatenate([[0], np.cumsum(pcnt)]).astype(np.int64)
    return ko, kt, pnode, prule, pcnt, poff


def total_events(case, t0, t1):
    """node events of the window (every node's list), without the lists"""
    return int(_pair_counts(case, t0, t1)[5][-1])


@functools.lru_cache(maxsize=3)
def _expected(name, t0, t1):
    case = CASES[name]()
    ko, kt, pnode, prule, pcnt, poff = _pair_counts(case, t0, t1)
    node_off = poff[np.searchsorted(pnode, np.arange(case.n_nodes + 1))]
    total = int(poff[-1])
    idx = np.repeat(ko[case.kind[prule]] - poff[:-1], pcnt) + np.arange(total, dtype=np.int64)
    out = node_off, kt[idx], np.repeat(prule, pcnt).astype(np.int32)
    for a in out:
        a.setflags(write=False)
    return out


def expected(case, t0=None, t1=None):
    """The whole per-node CSR of the window (the case's own by default) in
    rule order: (node_off int64 [N+1], time int64 [E], rule int32 [E]).
    Shared between callers and read-only."""
    t0, t1 = (case.t0, case.t1) if t0 is None else (t0, t1)
    return _expected(case.name, int(t0), int(t1))


@functools.lru_cache(maxsize=3)
def _expected_by_time(name, t0, t1):
    out = by_time(CASES[name](), _expected(name, t0, t1), t0)
    for a in out:
        a.setflags(write=False)
    return out


def expected_by_time(case, t0=None, t1=None):
    """expected() with every node's list in (time, rule) order; shared and read-only"""
    t0, t1 = (case.t0, case.t1) if t0 is None else (t0, t1)
    return _expected_by_time(case.name, int(t0), int(t1))


def by_time(case, csr, t0):
    """csr with every node's list in (time, rule) order: a stable sort by time
    within each node of the rule-ordered lists"""
    node_off, time, rule = csr
    node = np.repeat(np.arange(case.n_nodes, dtype=np.int64), np.diff(node_off))
    rel = time - t0
    assert len(rel) == 0 or (int(rel.min()) > 0 and int(rel.max()) < 1 << 16)  # (the windows in time order are short)
    o = _stable_by(rel, 1 << 16)  # equal times stay in rule order
    o = o[_stable_by(node[o], case.n_nodes)]
    return node_off, time[o], rule[o]


Segments = namedtuple("Segments", "pairs events start")


def segments(case, t0=None, t1=None):
    """per (node, band) segment, [N, K]: its pairs, its events, and the
    position of its first event in the whole output"""
    t0, t1 = (case.t0, case.t1) if t0 is None else (t0, t1)
    _, _, pnode, prule, pcnt, _ = _pair_counts(case, t0, t1)
    NK = case.n_nodes * case.K
    seg = pnode * case.K + prule // B
    ev = np.bincount(seg, weights=pcnt, minlength=NK).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(ev)[:-1]]).astype(np.int64)
    shape = (case.n_nodes, case.K)
    return Segments(np.bincount(seg, minlength=NK).reshape(shape), ev.reshape(shape), start.reshape(shape))


def record_x(case, t0=None, t1=None):
    """For every pair whose rule's fires form an arithmetic progression (one
    fire: stride 1, as k_rule_info has it): x = first fire - t0 - d * stride,
    d the events of the pair's segment in front of it -- the value a segment
    record holds when it fits 32 bits.  -> (x int64 [pairs], progression mask)"""
    t0, t1 = (case.t0, case.t1) if t0 is None else (t0, t1)
    ko, kt, pnode, prule, pcnt, poff = _pair_counts(case, t0, t1)
    nk = len(case.kinds)
    stride, first = np.zeros(nk, np.int64), np.zeros(nk, np.int64)
    for k in range(nk):
        f = kt[ko[k]:ko[k + 1]]
        if len(f) == 0:
            continue
        d = np.diff(f)
        first[k] = f[0] - t0
        stride[k] = 1 if len(f) == 1 else (int(d[0]) if (d == d[0]).all() else 0)
    seg = segments(case, t0, t1)
    d = poff[:-1] - seg.start.ravel()[pnode * case.K + prule // B]
    pk = case.kind[prule]
    prog = (pcnt > 0) & (stride[pk] > 0)
    return first[pk] - d * stride[pk], prog
