"""The fire-profile kernels (cg_profile.hip) against the host model
(profile_model.py) at the sizes where their loops change path: exact equality
of whole arrays, the first differing (row, bucket) named.

A rule set here is a base set of K rules picked R times (rule r = base rule
pick[r]); the base set's fire lists come from one oracle expansion per module
(profile_cases.utc_base / zone_base) and every expectation is a gather or a
K-wide integer product of it.  What makes a wrong index visible is asserted
with every case (visible()):

  * every base row is picked at least once, and pick[i] != pick[i+1];
  * at least a fifth of the neighbouring picked rows differ as rows of the
    case's own matrix, so a read one row off over any 50 rows goes unseen with
    probability under 0.8^50 = 1.5e-5 -- the UTC base has more than half of its
    rows pairwise distinct over its horizon (test_profile_model.py), but one
    60-s bucket can hold only a handful of distinct counts, and 24 half-hour
    buckets tell apart 36 of the zone base's 202 rows, so "half of the rows
    distinct" cannot hold in each case and this weaker, sufficient form does;
  * the rows on a block's or the matrix's last place, where a single row can
    be lost, are planted with rules that fire in every bucket;
  * with B >= 2 the expected totals are not all equal; with B = 1 the one
    expected column is not constant.
"""
import numpy as np
import pytest

import join_model as JM
import profile_cases as PC
import profile_model as PM
from common import product_zone
from cronsun_amd import _lib, cron
from join_cases import nid_rules_csr

pytestmark = pytest.mark.gpu

STRIDE = 4096 * 256  # k_profile_rules' grid cap in cells, k_profile_walk's in rules


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


# ---------------------------------------------------------------- helpers --
_parsed = {}


def upload_picked(eng, base, pick):
    """The rule set base.specs[pick], uploaded from one array of cg_schedule."""
    if id(base) not in _parsed:
        barr, status = cron.parse_batch(base.specs, threads=8)
        assert not np.any(status)
        _parsed[id(base)] = barr
    barr = _parsed[id(base)]
    a = np.ascontiguousarray(np.ctypeslib.as_array(barr)[:base.K][pick])
    return eng.upload_c((barr._type_ * len(pick)).from_buffer(a), len(pick))


def plant(pick, where):
    """pick with pick[i] = k for (i, k) in where, neighbours kept different."""
    K = int(pick.max()) + 1
    for i, k in where.items():
        pick[i] = k
    for i in where:
        for j in (i - 1, i + 1):
            if 0 <= j < len(pick) and j not in where and pick[j] == pick[i]:
                around = {int(pick[x]) for x in (j - 1, j + 1) if 0 <= x < len(pick)}
                pick[j] = next(v for v in range(K) if v not in around)
    return pick


def same(what, got, exp, row="rule", first_row=0):
    """Exact equality of two arrays; the first differing (row, bucket) named."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not np.array_equal(got, exp):
        at = [int(x[0]) for x in np.nonzero(got != exp)]
        where = f"{row} {first_row + at[0]} bucket {at[1]}" if got.ndim == 2 else f"bucket {at[0]}"
        raise AssertionError(f"{what}: {where}: {int(got[tuple(at)])} vs {int(exp[tuple(at)])}")


def neighbours_differ(m, seq):
    """At least a fifth of the neighbours in the sequence of base rules seq
    differ as rows of m."""
    label = np.unique(m, axis=0, return_inverse=True)[1].ravel()[seq]  # equal labels: equal rows
    return 5 * int((label[1:] != label[:-1]).sum()) >= len(seq) - 1


def visible(m, pick, dense_rows=()):
    """The conditions of the module docstring for one case; -> expected totals."""
    K, B = m.shape
    assert len(np.unique(pick)) == K and (pick[1:] != pick[:-1]).all()
    assert neighbours_differ(m, pick)
    for r in dense_rows:
        assert m[pick[r]].all(), r
    tot = PM.totals(m, pick)
    assert len(np.unique(tot)) > 1 if B >= 2 else len(np.unique(m[:, 0])) > 1
    return tot


def check_profile(eng, sp, base, pick, w, B, what, dense_rows=(), loc=None):
    """Engine.profile on the picked set: rule matrix, totals, row sums."""
    loc = loc or product_zone(base.zone)
    m = base.matrix(w, B)
    exp, tot = m[pick], visible(m, pick, dense_rows)
    rules, totals = eng.profile(sp, loc, base.t0, w, B)
    same(f"{what} rule matrix", rules, exp)
    same(f"{what} totals", totals, tot)
    count = eng.count(sp, loc, base.t0, base.t0 + w * B)
    assert np.array_equal(rules.sum(axis=1, dtype=np.int64), count), what
    return rules, totals


# ----------------------------------------------- a. totals, packing sweep --
@pytest.mark.parametrize("R", [4095, 4096, 4097, 8193])
def test_totals_blocks_and_row_packing(eng, R):
    """k_profile_totals' 4096-row blocks: one block short of full, full, two
    blocks with a single row in the second, three with one row in the third;
    at every B the tile_lane packing on both sides of its steps (64 / B rows a
    wave: 64, 32, 21, 3 | 2 at 21 | 22, 2 | 1 at 32 | 33, one row with one idle
    lane at 63, 64 | 65 and 127..129 across the second and third bucket tile).
    The last row of the set and of the first block fire in every bucket
    (every-second; seconds 7, 30, 45), so a dropped edge row changes every
    total.  w = 60."""
    base = PC.utc_base()
    pick = PM.make_pick(base.K, R, seed=R)
    where = {R - 1: base.specs.index("* * * * * *")}
    if R > 4096:
        where[4095] = base.specs.index("7,30,45 * * * * *")
    plant(pick, where)
    sp = upload_picked(eng, base, pick)
    for B in (1, 2, 3, 21, 22, 32, 33, 63, 64, 65, 127, 128, 129):
        check_profile(eng, sp, base, pick, 60, B, f"R={R} B={B}", dense_rows=where)
    sp.free()


# ------------------------------------------------------ b. the cell stride --
@pytest.mark.parametrize("R,B,w,dr,db", [(20_000, 130, 60, 8065, 126), (25_000, 130, 60, 8065, 126),
                                         (1_025, 4095, 20, 256, 256), (STRIDE + 77, 3, 3600, 349_525, 1),
                                         (5_000, 1000, 13, 1048, 576), (STRIDE + 77, 1, 20 * 4096, STRIDE, 0)])
def test_rule_matrix_cell_stride(eng, R, B, w, dr, db):
    """k_profile_rules past its 4096-block cap: a lane advances (rule, bucket)
    by (dr, db) with a carry.  20 000 x 130 (2.5 trips) and 25 000 x 130 (3.1
    trips: the same B with cells >= 3 * 2^20), 1 025 x 4095 (the carry fires
    on every trip), 2^20 + 77 rows x 3 (257 totals blocks, rows 21 abreast),
    5 000 x 1000, and 2^20 + 77 rows x 1 (db = 0: a lane's second trip is one
    of the last 77 rows).  The every-second rule is the last row."""
    assert (STRIDE // B, STRIDE % B) == (dr, db)
    if db:
        assert R * B >= 3 * STRIDE or (R, B) == (20_000, 130)
    base = PC.utc_base()
    pick = plant(PM.make_pick(base.K, R, seed=R + B), {R - 1: base.specs.index("* * * * * *")})
    sp = upload_picked(eng, base, pick)
    check_profile(eng, sp, base, pick, w, B, f"R={R} B={B}", dense_rows=[R - 1])
    sp.free()


# ------------------------------------------------- c. the walk's grid cap --
def test_walk_past_grid_cap(eng):
    """k_profile_walk's grid-stride loop: 2^20 + 333 rules of the zone base in
    Australia/Lord_Howe, 24 buckets of 1800 s from six hours before the
    transition of 2026-04-04 15:00 UTC (a 30-minute shift: walked runs), every
    cell against base[pick].  That walked runs exist shows in the walk kernel's time, which
    must exceed the same two events with no kernel between them (a UTC call).
    The last 333 rows are the walk's second trip: the last row is every-second
    and row 2^20 is the rule with most fires in the two buckets at the
    transition."""
    base = PC.zone_base()
    w, B, R = 1800, 24, STRIDE + 333
    m = base.matrix(w, B)
    tables = np.array([not s.startswith("@every") and s != "* * * * * *" for s in base.specs])
    busy = int(np.argmax(m[:, 11:13].sum(axis=1) * tables))  # (an @every rule is never walked)
    assert m[busy, 11:13].all()
    pick = plant(PM.make_pick(base.K, R, seed=R), {R - 1: base.specs.index("* * * * * *"), STRIDE: busy})
    sp = upload_picked(eng, base, pick)
    check_profile(eng, sp, base, pick, w, B, "walk", dense_rows=[R - 1])
    walk_ms = eng.profile_kernel_times()[1]
    eng.profile(sp.slice(0, 1000), product_zone("UTC"), base.t0, w, B)
    idle_ms = eng.profile_kernel_times()[1]
    print(f"k_profile_walk {walk_ms:.4f} ms, no launch {idle_ms:.4f} ms")
    assert walk_ms > 0 and walk_ms > idle_ms
    sp.free()


# ------------------------------------- d. node lists at the chunk edges --
N_D, R_D = 1030, 60_000
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 335, 336, 337, 511, 512, 513, 1023, 1024, 1025, 1536, 1537, 40_000]


def planted_join(R, N, lens, seed):
    """A rule set (NodeIDs only) whose node n runs lens[n] random rules:
    (rin, nt_off, nt_rule)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    nt_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    lists = [np.sort(rng.choice(R, int(n), replace=False)) for n in lens]
    nt_rule = (np.concatenate(lists) if nt_off[-1] else np.zeros(0)).astype(np.int32)
    node = np.repeat(np.arange(N, dtype=np.int32), lens)
    order = np.lexsort((node, nt_rule))
    rn_off = np.concatenate([[0], np.cumsum(np.bincount(nt_rule, minlength=R))]).astype(np.int64)
    rn_nodes = node[order]
    off, rule = JM.transpose(rn_off, rn_nodes, N)
    assert np.array_equal(off, nt_off) and np.array_equal(rule, nt_rule)
    return nid_rules_csr(N, rn_off, rn_nodes), nt_off, nt_rule


_node_case = {}


def node_case():
    if not _node_case:
        rng = np.random.default_rng(77)
        lens = rng.integers(0, 41, N_D)
        lens[0], lens[N_D - 1], lens[N_D - 2] = 0, 40_000, 1537
        lens[1023], lens[1024] = 1024, 1025  # two heavy nodes across the chunk scan's 1024-element tile
        spread = [n for n in LENGTHS if n not in (40_000, 1537)] + [1024, 1025, 0]
        for i, n in enumerate(spread):
            lens[40 + 47 * i] = n
        assert 40 + 47 * (len(spread) - 1) < 1023 and set(LENGTHS) <= set(lens.tolist())
        base = PC.utc_base()
        _node_case["v"] = (PM.make_pick(base.K, R_D, seed=R_D), lens) + planted_join(R_D, N_D, lens, 78)
    return _node_case["v"]


def check_per_node(eng, sp, dr, base, pick, nt_off, nt_rule, w, B, what, full=True):
    """One per-node call: node matrix against W @ base (and, at B <= 65,
    against segment sums of the copied rule matrix), rule matrix, totals."""
    m = base.matrix(w, B)
    exp, tot = m[pick], PM.totals(m, pick)
    nodes = eng.profile_per_node(sp, product_zone(base.zone), base.t0, w, B, dr, _lib.EXCLUDE_NONE)
    same(f"{what} node matrix", nodes, PM.node_matrix_tiled(nt_off, nt_rule, pick, m), "node")
    rules = eng.profile_rules()
    if full:
        same(f"{what} rule matrix", rules, exp)
    if B <= 65:
        same(f"{what} node matrix (segment sums)", nodes, PM.node_matrix(nt_off, nt_rule, rules), "node")
    same(f"{what} totals", eng.profile_totals(), tot)
    return nodes


@pytest.mark.parametrize("B", [1, 3, 64, 65, 130])
def test_node_lists_at_chunk_and_unroll_edges(eng, B):
    """60 000 rules on 1 030 nodes with planted list lengths: 0, 1; 15 | 16 |
    17 (one round of four load pairs at B >= 64); 335 | 336 | 337 (one round at
    B = 3, 84 rows a block); 255..257; 511 | 512 | 513 (one chunk | two); 1023
    | 1024 | 1025 and 1536 | 1537 (two | three | four chunks); 40 000 (79
    chunks).  Node 0 is empty and the last two nodes are heavy (the ends of
    the chunk -> node search); nodes 1023 and 1024, both heavy, sit on either
    side of the chunk scan's tile; the other nodes run 0-40 rules.  At B = 1
    only the tail loop runs.  The call is then repeated on the cached join and
    must give the same matrix."""
    pick, lens, rin, nt_off, nt_rule = node_case()
    base = PC.utc_base()
    m = base.matrix(60, B)
    visible(m, pick)
    assert neighbours_differ(m, pick[nt_rule])  # ... and so do the rules next to each other in a node's list
    sp, dr = upload_picked(eng, base, pick), eng.upload_rules(rin)
    nodes = check_per_node(eng, sp, dr, base, pick, nt_off, nt_rule, 60, B, f"B={B}")
    assert not nodes[0].any() and nodes[N_D - 1].any() and nodes[N_D - 2].any()
    assert eng.profile_kernel_times()[3] > 0
    again = eng.profile_per_node(sp, product_zone("UTC"), base.t0, 60, B, dr, _lib.EXCLUDE_NONE)
    assert eng.profile_kernel_times()[3] == 0  # the cached join
    same(f"B={B} repeated call", again, nodes, "node")
    dr.free()
    sp.free()


@pytest.mark.parametrize("B", [3, 65])
def test_one_node_and_no_pairs(eng, B):
    """One node with every rule (118 chunks, the search over a single node),
    one node with no rule, and five nodes of a set without any pair: zero
    rows, the rule matrix and totals as ever."""
    base = PC.utc_base()
    pick = node_case()[0]
    sp = upload_picked(eng, base, pick)
    every = np.arange(R_D + 1, dtype=np.int64)
    none = np.zeros(R_D + 1, dtype=np.int64)
    for N, rn_off, rn_nodes in ((1, every, np.zeros(R_D, np.int32)), (1, none, np.zeros(0, np.int32)),
                                (5, none, np.zeros(0, np.int32))):
        nt_off, nt_rule = JM.transpose(rn_off, rn_nodes, N)
        dr = eng.upload_rules(nid_rules_csr(N, rn_off, rn_nodes))
        nodes = check_per_node(eng, sp, dr, base, pick, nt_off, nt_rule, 60, B, f"N={N} nnz={len(rn_nodes)} B={B}",
                               full=False)
        assert nodes.shape == (N, B) and nodes.any() == bool(len(rn_nodes))
        if len(rn_nodes):
            same("the node with every rule", nodes[0], eng.profile_totals())
        dr.free()
    sp.free()


# ----------------------------------------------------- e. past 2^32 cells --
def test_past_2_to_32_cells():
    """R = 2^20 + 3 rules x 4096 buckets of 20 s: 2^32 + 3 * 4096 cells, 17 GB
    of rule matrix; three nodes, rule r on node r % 3 (683 chunks each).  The
    rule matrix is compared on the device, 65 536 rows (1 GiB) at a time,
    through the torch views; totals and node matrix on the host; the host copy
    at the rows that hold cells 2^31 - 1 | 2^31 and 2^32 - 1 | 2^32 and at the
    last three rows.  About half a second on an MI355X (0.3 s of it the host
    model), after the import of torch."""
    import torch
    from cronsun_amd.engine import Engine
    base = PC.utc_base()
    w, B, R, N = 20, 4096, STRIDE + 3, 3
    assert R * B == 2**32 + 3 * 4096
    m = base.matrix(w, B)
    pick = plant(PM.make_pick(base.K, R, seed=R), {R - 1: base.specs.index("* * * * * *")})
    tot = visible(m, pick, [R - 1])
    rn_off, rn_nodes = np.arange(R + 1, dtype=np.int64), (np.arange(R) % N).astype(np.int32)
    exp_nodes = PM.node_matrix_tiled(*JM.transpose(rn_off, rn_nodes, N), pick, m)
    eng = Engine(0)
    try:
        sp, dr = upload_picked(eng, base, pick), eng.upload_rules(nid_rules_csr(N, rn_off, rn_nodes))
        rules_t, totals_t, nodes_t = eng.profile_per_node_device(sp, product_zone("UTC"), base.t0, w, B, dr,
                                                                 _lib.EXCLUDE_NONE)
        assert tuple(rules_t.shape) == (R, B) and rules_t.dtype == torch.int32 and rules_t.is_contiguous()
        assert rules_t.data_ptr() == eng.profile_result_device()[0]
        dev = rules_t.device
        base_t, pick_t = torch.from_numpy(m).to(dev), torch.from_numpy(pick).to(dev)
        for lo in range(0, R, 65536):
            hi = min(R, lo + 65536)
            exp_t = base_t[pick_t[lo:hi]]
            if not torch.equal(rules_t[lo:hi], exp_t):
                same("rule matrix", rules_t[lo:hi].cpu().numpy(), exp_t.cpu().numpy(), first_row=lo)
            del exp_t
        same("totals", totals_t.cpu().numpy(), tot)
        same("node matrix", nodes_t.cpu().numpy(), exp_nodes, "node")
        del rules_t, totals_t, nodes_t, base_t, pick_t
        for edge in (2**31, 2**32, R * B):  # rows first .. first + 2 hold cells edge - 1 | edge
            first = min(edge // B - 2, R - 3)
            assert first * B < edge - 1 and edge <= (first + 3) * B
            same(f"host copy of rows {first}..{first + 2}", eng.profile_rules(first, 3), m[pick[first:first + 3]])
        same("host copy of the node matrix", eng.profile_nodes(), exp_nodes, "node")
    finally:
        eng.close()
        torch.cuda.empty_cache()
