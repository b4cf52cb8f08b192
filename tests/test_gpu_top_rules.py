"""Top rules of a profile bucket on the GPU (cg_profile_top_rules_*): for every
node, or for the cluster-wide row, the k rules with the largest cells in one
bucket of the readable profile, against the host model (top_rules_model.py)
over the oracle's rule matrix (profile_cases / inflight_model) and the
oracle's Job.Cmds filter (O.node_rules).  Exact integer equality throughout;
the first differing (row, position) is named.  The oracle's fire lists are
built once per module."""
import numpy as np
import pytest

import inflight_model as IM
import oracle_lib as O
import profile_cases as PC
import profile_model as PM
import top_rules_model as TM
from common import oracle_zone, product_zone
from cronsun_amd import _lib, cron
from join_cases import nid_rules_csr

pytestmark = pytest.mark.gpu

KS = (1, 7, 64)
CHUNK = 512  # candidates per chunk of a row (kNodeChunk)


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


# ---------------------------------------------------------------- helpers --
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def set_lists(name):
    """The oracle's fire lists of rule_set(name) over the longest horizon of
    the node cases (65 minutes)."""
    return cached(("lists", name), lambda: O.expand_batch(O.sched_array(PC.rule_set(name)[2]), PC.T0_UTC,
                                                         PC.T0_UTC + 3900, oracle_zone("UTC")))


def cycle(values, n):
    return np.array([values[i % len(values)] for i in range(n)], dtype=np.int64)


def expected_matrix(name, w, B, inflight):
    """(rule matrix int32 [R, B], durations or None) of rule_set(name)."""
    def make():
        off, times = set_lists(name)
        if not inflight:
            return PM.bin_fires(off, times, PC.T0_UTC, w, B), None
        dur = cycle(IM.duration_cycle(w), len(off) - 1)
        return IM.inflight_from_lists(off, times, PC.T0_UTC, w, B, IM.seconds(dur)), dur
    return cached(("matrix", name, w, B, inflight), make)


def node_lists(name, mode):
    rin = PC.rule_set(name)[0]
    return cached(("join", name, mode), lambda: O.node_rules(rin, mode, np.arange(rin.n_nodes)))


def seeded_buckets(N, B, seed):
    return np.random.default_rng(seed).integers(0, B, N).astype(np.int32)


def upload(eng, specs):
    return eng.upload([cron.Parse(s) for s in specs])


def run_profile(eng, sp, dr, w, B, dur, mode, t0=PC.T0_UTC):
    utc = product_zone("UTC")
    if dur is None:
        return eng.profile_per_node(sp, utc, t0, w, B, dr, mode)
    return eng.inflight_per_node(sp, utc, t0, w, B, dur, dr, mode)


def einval(call, *needles):
    with pytest.raises(_lib.CgError) as e:
        call()
    assert e.value.code == _lib.CG_EINVAL, e.value.msg
    for s in needles:
        assert s in e.value.msg, e.value.msg
    return e.value.msg


# ------------------------------------------------- 1. nodes against the oracle --
WB = [(60, 65), (3600, 1), (7, 520)]


@pytest.mark.parametrize("inflight", [False, True], ids=["starts", "inflight"])
@pytest.mark.parametrize("mode", [_lib.EXCLUDE_NONE, _lib.EXCLUDE_CUMULATIVE])
@pytest.mark.parametrize("name", ["nodes48", "keys3"])
def test_nodes_against_the_oracle(eng, name, mode, inflight):
    """3000 one-rule jobs on 48 nodes / 400 jobs whose rules repeat Cmd keys,
    each with a node every rule names (its list is split into chunks) and a
    node no rule reaches; 65 one-minute buckets, one bucket, 520 of 7 s (B
    below and above a wave).  Every node is ranked at its peak bucket and at
    a seeded bucket, with k = 1, 7 and 64: all five columns equal the model,
    the peak ranking's bucket column is profile_node_peaks', and the lists of
    rows with n_contrib <= k sum to the node-matrix cell.  For every k some
    row's cut falls inside a run of equal counts, and some row has more than
    64 contributors."""
    rin, specs, _ = PC.rule_set(name)
    N = rin.n_nodes
    roff, rules = node_lists(name, mode)
    assert roff[N - 1] - roff[N - 2] > CHUNK and roff[N] == roff[N - 1]  # the heavy node, the empty one
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    ties, big = {k: [] for k in KS}, False
    for w, B in WB:
        matrix, dur = expected_matrix(name, w, B, inflight)
        nodes = run_profile(eng, sp, dr, w, B, dur, mode)
        peak, peak_at = eng.profile_node_peaks()
        assert np.array_equal(peak_at, IM.peaks(PC.oracle_node_matrix(rin, mode, matrix)[0])[1])
        for k in KS:
            for what, arg, at in (("peak", None, peak_at), ("seeded", seeded_buckets(N, B, 100 * k + B), None)):
                at = arg if at is None else at
                got = eng.profile_top_rules(k, arg)
                exp = TM.top_rules(matrix, roff, rules, at, k)
                TM.same(f"{name} mode {mode} w={w} B={B} k={k} at the {what} buckets", got, exp)
                rule, count, n_listed, n_contrib, bucket = got
                assert np.array_equal(bucket, at)
                whole = n_contrib <= k
                assert np.array_equal(count[whole].sum(axis=1, dtype=np.int64), nodes[np.arange(N), at][whole])
                assert n_listed[N - 1] == 0 and n_contrib[N - 1] == 0 and (rule[N - 1] == -1).all()  # the empty node
                ties[k] += TM.tie_at_cut(matrix, roff, rules, at, k)
                big = big or bool((n_contrib > 64).any())
        assert eng.profile_top_rules_ms()[2] == np.maximum(1, -(-np.diff(roff) // CHUNK)).sum() > N  # a split row
    assert all(ties[k] for k in KS) and big, (ties, big)
    dr.free()
    sp.free()


# --------------------------------- 2. split rows, the insertion path's extremes --
R2 = 20_011
W2, B2 = 3600, 8


@pytest.fixture(scope="module")
def every_second(eng):
    """R2 every-second rules, one-rule jobs, on 3 nodes: node 0 named by every
    rule, node 1 by the odd rules, node 2 by none."""
    barr, status = cron.parse_batch(["* * * * * *"], threads=1)
    assert not np.any(status)
    a = np.ascontiguousarray(np.repeat(np.ctypeslib.as_array(barr)[:1], R2))
    sp = eng.upload_c((barr._type_ * R2).from_buffer(a), R2)
    lens = 1 + (np.arange(R2) % 2)
    nid_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nids = np.zeros(int(nid_off[-1]), dtype=np.int32)
    nids[nid_off[1:][1::2] - 1] = 1  # the second entry of every odd rule
    dr = eng.upload_rules(nid_rules_csr(3, nid_off, nids))
    yield sp, dr
    dr.free()
    sp.free()


def closed_form(cells, k):
    """The three rows from the cells [R2] of bucket 7: node 0 all rules, node 1
    the odd ones, node 2 none -- by a plain lexsort, no model."""
    out = []
    for cand in (np.arange(R2), np.arange(1, R2, 2), np.zeros(0, dtype=np.int64)):
        order = cand[np.lexsort((cand, -cells[cand]))][:k] if len(cand) else cand
        pad = k - len(order)
        out.append((np.concatenate([order, np.full(pad, -1)]), np.concatenate([cells[order], np.zeros(pad)]),
                    len(order), len(cand)))
    i32 = lambda i, shape: np.array([row[i] for row in out], dtype=np.int32).reshape(shape)  # noqa: E731
    return i32(0, (3, k)), i32(1, (3, k)), i32(2, 3), i32(3, 3), np.full(3, B2 - 1, dtype=np.int32)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
def test_split_rows(eng, every_second, order, k):
    """In flight at the last of 8 one-hour edges, an every-second rule running
    d seconds has the cell min(d, 28800).  d = r + 1: cells strictly ascending
    in rule order, every candidate enters the list; d = R - r: strictly
    descending, none enters after the first 64; d = 5 everywhere: all cells
    equal, so the rule index alone decides (node 0: rules 0..k-1, node 1: 1,
    3, 5, ...).  Node 0's 20 011 candidates span 40 chunks."""
    sp, dr = every_second
    r = np.arange(R2, dtype=np.int64)
    d = {"ascending": r + 1, "descending": R2 - r, "equal": np.full(R2, 5, dtype=np.int64)}[order]
    nodes = eng.inflight_per_node(sp, product_zone("UTC"), PC.T0_UTC, W2, B2, d * 1000, dr, _lib.EXCLUDE_NONE)
    cells = np.minimum(d, W2 * B2)
    assert nodes[:, B2 - 1].tolist() == [int(cells.sum()), int(cells[1::2].sum()), 0]
    got = eng.profile_top_rules(k, np.full(3, B2 - 1, dtype=np.int32))
    TM.same(f"{order} k={k}", got, closed_form(cells, k))
    if order == "equal":
        assert got[0][0].tolist() == list(range(k)) and got[0][1].tolist() == list(range(1, 2 * k, 2))
    chunks = eng.profile_top_rules_ms()[2]
    assert chunks >= 3 + 2 and chunks == -(-R2 // CHUNK) + -(-(R2 // 2) // CHUNK) + 1
    assert eng.profile_top_rules_ms()[1] > 0  # the merge ran
    # ... and at the peak buckets: a row is at its peak from the first edge past its longest duration on,
    # with every cell what it is at the last edge
    exp = closed_form(cells, k)
    edges = W2 * (np.arange(B2) + 1)
    for n, cand in enumerate((r, r[1::2])):
        exp[4][n] = np.argmax(np.minimum(d[cand][:, None], edges[None, :]).sum(axis=0))
    exp[4][2] = 0
    assert exp[4][0] < B2 - 1
    TM.same(f"{order} k={k} at the peaks", eng.profile_top_rules(k), exp)


# ---------------------------------------------------------- 3. cluster-wide --
def test_cluster_wide(eng):
    """The 20 011-rule picked set of the in-flight identities test (many equal
    rows, so many ties), starts, 65 one-minute buckets, after Engine.profile
    with no node matrix: buckets 0, 1 and 64 with k = 64; the end of the row is
    reached; the per-node call is refused."""
    base = PC.utc_base()
    w, B, R = 60, 65, 20_011
    pick = PM.make_pick(base.K, R, seed=R)
    barr, status = cron.parse_batch(base.specs, threads=8)
    assert not np.any(status)
    a = np.ascontiguousarray(np.ctypeslib.as_array(barr)[:base.K][pick])
    sp = eng.upload_c((barr._type_ * R).from_buffer(a), R)
    matrix = base.matrix(w, B)[pick]
    rules, _ = eng.profile(sp, product_zone("UTC"), base.t0, w, B)
    assert np.array_equal(rules, matrix)
    off1, all_rules = TM.cluster_lists(R)
    for b in (0, 1, 64):
        got = eng.profile_top_rules_bucket(b, 64)
        TM.same(f"bucket {b}", got, TM.top_rules(matrix, off1, all_rules, [b], 64))
        assert got[3][0] > 64 and TM.tie_at_cut(matrix, off1, all_rules, [b], 64) == [0]
    assert eng.profile_top_rules_ms()[2] == -(-R // CHUNK)
    # The end of the row.  Rule 20 010 of this set is "0 18 0 * * 1-4", which fires in none of the 65 minutes
    # from 08:59:17, so no bucket has it as a contributor; the last rule that contributes anywhere is 20 009,
    # in the same, partly filled last chunk.  n_contrib counts it (test_cluster_wide_reaches_the_last_rule
    # lists the very last rule of a row).
    assert not matrix[R - 1].any()
    last = int(np.nonzero(matrix.any(axis=1))[0][-1])
    assert last == R - 2 and last // CHUNK == (R - 1) // CHUNK
    b = int(np.argmax(matrix[last]))
    assert last in TM.full_order(matrix, all_rules, b)[0]
    TM.same(f"bucket {b}, where rule {last} contributes", eng.profile_top_rules_bucket(b, 64),
            TM.top_rules(matrix, off1, all_rules, [b], 64))
    einval(lambda: eng.profile_top_rules(3), "no node matrix")
    # k = 1 with everything tied at the top: the smallest rule index
    got = eng.profile_top_rules_bucket(0, 1)
    TM.same("k = 1", got, TM.top_rules(matrix, off1, all_rules, [0], 1))
    sp.free()


def test_cluster_wide_reaches_the_last_rule(eng):
    """One rule past a chunk boundary (513 rules), the last one the only
    contributor of bucket 1 and the largest of bucket 0."""
    specs = ["0 0 * * * *"] * 512 + ["* * * * * *"]
    sp = upload(eng, specs)
    t0 = 1767225600 + 3600 - 60  # bucket 0 of 60 s ends on the hour, where the 512 hourly rules fire
    eng.profile(sp, product_zone("UTC"), t0, 60, 2)
    rule, count, n_listed, n_contrib, bucket = eng.profile_top_rules_bucket(1, 64)
    assert (n_listed[0], n_contrib[0], bucket[0]) == (1, 1, 1)
    assert rule[0].tolist() == [512] + [-1] * 63 and count[0].tolist() == [60] + [0] * 63
    rule, count, n_listed, n_contrib, bucket = eng.profile_top_rules_bucket(0, 3)
    assert rule[0].tolist() == [512, 0, 1] and count[0].tolist() == [60, 1, 1] and n_contrib[0] == 513
    assert eng.profile_top_rules_ms()[2] == 2
    sp.free()


# ------------------------------------------------- 4. staleness and lifetime --
def test_staleness_and_lifetime(eng):
    rin, specs, _ = PC.rule_set("keys3")
    w, B, k = 60, 65, 7
    matrix, _ = expected_matrix("keys3", w, B, False)
    roff, rules = node_lists("keys3", _lib.EXCLUDE_NONE)
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    utc = product_zone("UTC")
    nodes = eng.profile_per_node(sp, utc, PC.T0_UTC, w, B, dr, _lib.EXCLUDE_NONE)
    rule_matrix = eng.profile_rules()
    peaks = eng.profile_node_peaks()
    first = eng.profile_top_rules(k)
    TM.same("first ranking", first, TM.top_rules(matrix, roff, rules, peaks[1], k))
    # a ranking leaves the profile and the peaks as they were
    assert np.array_equal(eng.profile_rules(), rule_matrix) and np.array_equal(eng.profile_nodes(), nodes)
    again = eng.profile_node_peaks()
    assert np.array_equal(again[0], peaks[0]) and np.array_equal(again[1], peaks[1])
    # a per-node expansion on the same set and mode hits the cache: the ranking stands, byte for byte
    eng.expand_per_node_rules_device(sp, utc, PC.T0_UTC, PC.T0_UTC + 600, dr, _lib.EXCLUDE_NONE)
    second = eng.profile_top_rules(k)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    # ... in another mode it rebuilds the transpose under the profile
    eng.expand_per_node_rules_device(sp, utc, PC.T0_UTC, PC.T0_UTC + 600, dr, _lib.EXCLUDE_CUMULATIVE)
    einval(lambda: eng.profile_top_rules(k), "replaced")
    for a, b in zip(second, eng.profile_top_rules_copy()):  # the refusal left the result readable
        assert a.tobytes() == b.tobytes()
    off1, all_rules = TM.cluster_lists(len(specs))
    TM.same("cluster-wide under a replaced join", eng.profile_top_rules_bucket(3, k),
            TM.top_rules(matrix, off1, all_rules, [3], k))
    assert np.array_equal(eng.profile_rules(), rule_matrix) and np.array_equal(eng.profile_nodes(), nodes)
    # a new profile call drops the list
    eng.profile_per_node(sp, utc, PC.T0_UTC, w, B, dr, _lib.EXCLUDE_NONE)
    einval(eng.profile_top_rules_device, "no top-rules result")
    einval(eng.profile_top_rules_copy)
    TM.same("after the new profile", eng.profile_top_rules(k), first)
    dr.free()
    sp.free()


# ----------------------------------------------------------- 5. arguments --
def test_arguments(eng):
    rin, specs, _ = PC.rule_set("keys3")
    w, B, k = 60, 65, 7
    N = rin.n_nodes
    sp, dr = upload(eng, specs), eng.upload_rules(rin)
    eng.profile_per_node(sp, product_zone("UTC"), PC.T0_UTC, w, B, dr, _lib.EXCLUDE_NONE)
    at = seeded_buckets(N, B, 5)
    kept = eng.profile_top_rules(k, at)

    def still_readable():
        for a, b in zip(kept, eng.profile_top_rules_copy()):
            assert a.tobytes() == b.tobytes()
        assert eng.profile_top_rules_device()[5:] == (N, k)
    for bad_k in (0, 65, -1):
        einval(lambda: eng.profile_top_rules(bad_k, at), "k outside [1, 64]")
        einval(lambda: eng.profile_top_rules_bucket(0, bad_k), "k outside [1, 64]")
        still_readable()
    bad = at.copy()
    bad[[11, 40]] = B
    einval(lambda: eng.profile_top_rules(k, bad), "node 11:")
    bad = at.copy()
    bad[[9, 11]] = [-1, B]
    einval(lambda: eng.profile_top_rules(k, bad), "node 9:")
    einval(lambda: eng.profile_top_rules_bucket(B, k))
    einval(lambda: eng.profile_top_rules_bucket(-1, k))
    still_readable()
    einval(lambda: eng.profile_top_rules_copy(1, N), "row range")
    einval(lambda: eng.profile_top_rules_copy(-1, 1), "row range")
    einval(lambda: eng.profile_top_rules_copy(N, 1), "row range")
    with pytest.raises(ValueError):
        eng.profile_top_rules(k, at[:-1])
    still_readable()
    part = eng.profile_top_rules_copy(3, 5)
    for a, b in zip(kept, part):
        assert np.array_equal(a[3:8], b)
    assert all(len(x) == 0 for x in eng.profile_top_rules_copy(N, 0))
    dr.free()
    sp.free()


# ----------------------------------------------- 6. JobSet.node_peak_rules --
def test_jobset_node_peak_rules(eng):
    """Six jobs on two nodes and a node nothing runs on, an hour from 00:00:00
    in four 15-minute buckets.  na runs all six: 900 + 90 + 15 + 15 + 1 commands
    a bucket and one more in the last, where the hourly rule fires, so it
    peaks in bucket 3; the two minutely rules tie and the earlier rule leads.
    nb runs only jb's and jf's rules.  In flight with AvgTime 25 s, 120 s, 1
    ms and none: at every edge 25 of ja's starts and 2 of jd's, at the last
    also jf's."""
    from cronsun_amd.ingest import EtcdJobSet
    from cronsun_amd.model import Group, Job, JobRule, JobSet
    import json
    groups = {"all": Group("all", "", ["na", "nb"]), "a": Group("a", "", ["na"])}
    table = [("ja", "r-sec", "* * * * * *", "a", 25_000), ("jb", "r-10s", "*/10 * * * * *", "all", 0),
             ("jc", "r-min", "0 * * * * *", "a", 0), ("jd", "r-min2", "30 * * * * *", "a", 120_000),
             ("je", "r-odd", "0 7,22,37,52 * * * *", "a", 0), ("jf", "r-hour", "0 0 * * * *", "all", 1)]
    jobs = [Job(j, Rules=[JobRule(r, spec, [g], [], [])], AvgTime=avg) for j, r, spec, g, avg in table]
    t0 = 1767225600  # 2026-01-01 00:00:00 UTC: the buckets end at :15, :30, :45 and 01:00:00
    exp_a = (900 + 90 + 15 + 15 + 1 + 1, 3, [("ja", "r-sec", 900), ("jb", "r-10s", 90), ("jc", "r-min", 15),
                                              ("jd", "r-min2", 15), ("je", "r-odd", 1), ("jf", "r-hour", 1)])
    exp_b = (91, 3, [("jb", "r-10s", 90), ("jf", "r-hour", 1)])
    docs = [json.dumps({"id": j, "avg_time": avg, "rules": [{"id": r, "timer": spec, "gids": [g]}]})
            for j, r, spec, g, avg in table]
    gdocs = [json.dumps({"id": "all", "nids": ["na", "nb"]}), json.dumps({"id": "a", "nids": ["na"]})]
    for js in (JobSet(jobs, groups), EtcdJobSet(docs, gdocs, threads=2)):
        assert js.node_peak_rules(t0, 900, 4, engine=eng) == {"na": exp_a, "nb": exp_b}
        assert js.node_peak_rules(t0, 900, 4, k=3, engine=eng)["na"] == (exp_a[0], 3, exp_a[2][:3])
        flight, missing = js.node_peak_rules(t0, 900, 4, k=2, inflight=True, engine=eng)
        assert missing == 3
        assert flight["na"] == (25 + 2 + 1, 3, [("ja", "r-sec", 25), ("jd", "r-min2", 2)])
        assert flight["nb"] == (1, 3, [("jf", "r-hour", 1)])
    one = JobSet(jobs[:1], {"a": Group("a", "", ["na"]), "idle": Group("idle", "", ["nz"])})
    assert one.node_peak_rules(t0, 900, 4, engine=eng) == {"na": (900, 0, [("ja", "r-sec", 900)]), "nz": (0, 0, [])}
