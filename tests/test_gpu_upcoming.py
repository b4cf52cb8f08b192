"""cg_dispatcher_upcoming* against tests/upcoming_model.py (pinned on the CPU
by tests/test_upcoming_model.py): the next k entries in byTime order,
cluster-wide and per node.  Tables are @every delays drawn from seeded RNGs, so
the expected Next is now + d with no oracle call; "after wakes" goes through
dispatch_model.DispatchModel.  Every case compares slot, Next and Prev of every
listed entry, n_out and n_total, exactly."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, product_zone, random_spec
from cronsun_amd import _lib, cron
from dispatch_model import DispatchModel
from patch_common import World
from upcoming_model import NO_PROGRESS, node_rows, upcoming

pytestmark = pytest.mark.gpu

Z = O.ZERO_TIME
T0 = 1767225600  # 2026-01-01T00:00:00Z
DAY = 86400
KMAX = _lib.UPCOMING_MAX
TILE = 4096  # kUpTile of cg_upcoming.hip = kDispatchTile


@pytest.fixture(scope="module")
def eng():
    from cronsun_amd.engine import Engine
    return Engine(0)


def delay_table(eng, delays, now):
    """A dispatcher of @every rows started at `now` -> (dispatcher, next, prev)
    with next = now + delay, prev = zero."""
    d = np.asarray(delays, dtype=np.int64)
    zero = np.zeros(len(d), dtype=np.uint64)
    sp = eng.upload_soa(zero, zero, zero, zero, zero, zero, d * 10**9)
    disp = eng.dispatcher(sp, None, now)
    sp.free()
    return disp, now + d, np.full(len(d), Z, dtype=np.int64)


def check(d, nx, pv, k, until=None, rows=None, node=None, what=None):
    """One upcoming call against the model; -> the device's three columns."""
    n_out, n_total = d.upcoming_count(k, until, node)
    got = d.upcoming_copy(n_out)
    es, ea, eb, etot = upcoming(nx, pv, k, until, rows)
    ctx = (what, k, until, node)
    assert (n_out, n_total) == (len(es), etot), ctx
    for g, e, name in zip(got, (es, ea, eb), ("slot", "next", "prev")):
        assert g.dtype == e.dtype and np.array_equal(g, e), (ctx, name)
    ms, passes = d.upcoming_ms()
    assert len(ms) == 3 and 0 <= passes <= 11, ctx
    return got


def refused(code, fn, *a):
    with pytest.raises(_lib.CgError) as e:
        fn(*a)
    assert e.value.code == code, e.value


# 1. sizes around the wave and the tile
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5])
def test_sizes_around_wave_and_tile(eng, n):
    rng = np.random.default_rng(100 + n)
    delays = rng.integers(2, 5000, n)  # many equal Next values at the larger sizes
    first = int(rng.integers(0, n))
    delays[first] = 1
    d, nx, pv = delay_table(eng, delays, T0)
    assert d.effective == T0 + 1
    for k in sorted({1, 2, max(n - 1, 1), n, min(n + 1, KMAX)}):
        s, a, _ = check(d, nx, pv, k)
        if k == 1:
            assert s.tolist() == [first] and a.tolist() == [d.effective]
    d.free()


# 2. ties across the cut: the ties taken are the lowest slots
@pytest.mark.parametrize("last_tile_only", [False, True])
def test_ties_across_the_cut(eng, last_tile_only):
    rng = np.random.default_rng(2)
    tied = 5000  # two digit passes below the first bin
    if last_tile_only:
        # two tiles of later entries with the 100 earlier ones among them,
        # then one whole tile of ties
        n = 3 * TILE
        delays = rng.integers(tied + 1, 2 * tied, n)
        delays[2 * TILE:] = tied
        early = rng.choice(2 * TILE, 100, replace=False)
    else:
        n = 10100
        delays = np.full(n, tied, dtype=np.int64)
        early = rng.choice(n, 100, replace=False)
    delays[early] = rng.integers(1, 90, 100)
    d, nx, pv = delay_table(eng, delays, T0)
    for k in (100, 101, 4196, 4197):
        s, a, _ = check(d, nx, pv, k, what=last_tile_only)
        ties = s[a == T0 + tied]
        want = np.flatnonzero(nx == T0 + tied)[:len(ties)]
        assert len(ties) == min(k - 100, len(np.flatnonzero(nx == T0 + tied))) and np.array_equal(ties, want)
    check(d, nx, pv, 4197, until=T0 + tied)
    check(d, nx, pv, 101, until=T0 + tied - 1)
    d.free()


# 3. key width and sign: Next values 2^32 s apart, and on both sides of the epoch
@pytest.mark.parametrize("now", [T0, -1800])
def test_key_width_and_sign(eng, now):
    """cg_dispatcher_new accepts a `now` below 0 (any time within +-2^45 s), so
    the second table's Next values straddle the epoch."""
    rng = np.random.default_rng(3)
    n = 3000  # past the one-block sort: the wide keys go through two LSD rounds
    wide = 1193047 * 3600  # 1193047h, just over 2^32 s
    assert wide > 1 << 32
    delays = np.where(np.arange(n) % 2 == 0, 3600, wide) + rng.integers(0, 40, n)
    delays[7] = 600
    d, nx, pv = delay_table(eng, delays, now)
    assert d.effective == now + 600
    if now < 0:
        assert nx.min() < 0 < np.sort(nx)[1]
    for k in (1, 10, 1500, 1501, n):
        check(d, nx, pv, k)
    check(d, nx, pv, n, until=now + 3600 + 20)
    check(d, nx, pv, 5, until=now + wide + 3)
    d.free()


# 4. what is not firing
NEVER = "0 0 0 30 Feb ?"
APIA = ["0 0 12 * * *", "0 0 9 * * Sat", "@daily"]  # test_gpu_dispatch.py (e)
APIA_T0 = 1325030400


def test_not_firing_never_removed_skipped(eng):
    rng = np.random.default_rng(4)
    n = 700
    delays = rng.integers(1, 3000, n)
    never = rng.choice(n, 60, replace=False)
    scheds = [cron.Every(int(x) * 10**9) for x in delays]
    for i in never:
        scheds[i] = cron.Parse(NEVER)
    d = eng.dispatcher(scheds, None, T0)
    nx = T0 + delays
    nx[never] = Z
    removed = rng.choice(np.setdiff1d(np.arange(n), never), 50, replace=False)
    d.remove(removed)
    nx[removed] = Z
    d.set([n + 40, n + 41], [cron.Every(7 * 10**9), cron.Parse(NEVER)], T0)  # slots n .. n+39 skipped
    nx = np.concatenate([nx, np.full(40, Z), [T0 + 7, Z]])
    pv = np.full(len(nx), Z, dtype=np.int64)
    snx, spv, live = d.snapshot()
    assert np.array_equal(snx, nx) and np.array_equal(spv, pv) and not live[n:n + 40].any()
    firing = n - 60 - 50 + 1
    for k in (1, firing - 1, firing, firing + 1, len(nx), KMAX):
        s, _, _ = check(d, nx, pv, k)
    assert d.upcoming_total == firing and len(s) == firing
    assert not np.isin(s, np.concatenate([never, removed, np.arange(n, n + 40), [n + 41]])).any()
    # nothing firing at all: CG_OK with zeros
    d.remove(np.flatnonzero(nx != Z))
    assert d.upcoming_count(10) == (0, 0)
    assert [len(x) for x in d.upcoming_copy(0)] == [0, 0, 0]
    d.free()
    # an empty table
    e = eng.dispatcher([], None, T0)
    assert e.upcoming_count(10) == (0, 0)
    e.free()


def test_not_firing_stuck_slots(eng):
    """The stuck-slot state of test_gpu_dispatch.py's test_stuck_entry_at_new:
    cg_dispatcher_new names slot 1 and hands the table back, slots 1 and 3 hold
    the no-progress value; they are neither listed nor counted."""
    L = _lib
    scheds = [cron.Parse(s) for s in (APIA[0], APIA[1], APIA[2], APIA[1], "@every 90s")]
    sp = eng.upload(scheds)
    z = product_zone("Pacific/Apia")  # (kept: the handle dies with the Location)
    h = C.c_void_p()
    rc = L.lib().cg_dispatcher_new(eng._h, sp._h, z.handle, APIA_T0, C.byref(h))
    assert rc == L.CG_ERANGE and "entry 1:" in L.last_error() and h
    from cronsun_amd.engine import Dispatcher
    d = Dispatcher(eng, h)
    nx, pv, _ = d.snapshot()
    assert nx[[1, 3]].tolist() == [NO_PROGRESS] * 2 and nx[4] == APIA_T0 + 90
    for k in (1, 3, 5):
        s, _, _ = check(d, nx, pv, k)
    assert sorted(s.tolist()) == [0, 2, 4] and d.upcoming_total == 3
    d.free()
    sp.free()


# 5. until
def test_until(eng):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 77
    delays = rng.integers(51, 4000, n)
    delays[rng.choice(n, 9, replace=False)] = 50
    d, nx, pv = delay_table(eng, delays, T0)
    eff = d.effective
    assert eff == T0 + 50
    assert d.upcoming_count(n, until=eff - 1) == (0, 0)
    assert d.upcoming_count(n, until=-(1 << 63)) == (0, 0)
    s, _, _ = check(d, nx, pv, n, until=eff)
    assert len(s) == 9
    for until in (eff + 1, T0 + 1000, T0 + 2025, T0 + 3999, T0 + 4000):
        for k in (1, 300, 3000, n):
            check(d, nx, pv, k, until=until)
    assert d.upcoming_count(300, until=T0 + 2025) == (300, int((nx <= T0 + 2025).sum()))
    # until = effective and k >= n: the due list of the wake made right after
    due, _ = d.fire(eff)
    assert np.array_equal(s, due)
    got = np.empty(len(due), dtype=np.int32)
    assert _lib.lib().cg_dispatcher_due(d._h, 0, len(due), got.ctypes.data) == 0
    assert np.array_equal(got, s)
    d.free()


# 6. after wakes and edits
def test_after_wakes_and_edits(eng):
    rng = np.random.default_rng(6)
    specs = []
    while len(specs) < 250:
        s = random_spec(rng)
        if O.parse(s)[1] is None:
            specs.append(s)
    delays = [int(x) for x in rng.integers(1, 600, 350)]
    n = len(specs) + len(delays)
    m = DispatchModel(oracle_zone("UTC"), list(oracle_parse_all(specs)) + delays)
    m.start(T0)
    d = eng.dispatcher([cron.Parse(s) for s in specs] + [cron.Every(x * 10**9) for x in delays], None, T0)
    for w in range(10):
        e = m.effective()
        assert d.effective == e
        now = e + int(rng.choice([0, 0, 1, 61]))
        due, _ = d.fire(now)
        mdue, _ = m.fire(now)
        assert np.array_equal(due, mdue)
        for k in (1, 50, n):
            check(d, m.next, m.prev, k, what=w)
        check(d, m.next, m.prev, n, until=m.effective() + 30, what=w)
    assert (m.prev != Z).sum() > 10
    now = m.effective()
    new = ["@every 3s", specs[0], "@every 1h"]
    slots = [5, 300, n + 2]
    s_before, _, _ = check(d, m.next, m.prev, 20)
    d.set(slots, [cron.Parse(s) for s in new], now)
    m.set(slots, list(oracle_parse_all(new)), now)
    # the list describes the table before the set: refused until a new call
    refused(_lib.CG_EINVAL, d.upcoming_copy, 20)
    refused(_lib.CG_EINVAL, d.upcoming_device)
    s_after, _, _ = check(d, m.next, m.prev, 20)
    assert not np.array_equal(s_before, s_after) and d.upcoming_device()[3] == 20
    d.remove([5, 17])
    m.remove([5, 17])
    refused(_lib.CG_EINVAL, d.upcoming_copy, 20)
    for k in (1, 20, len(m)):
        check(d, m.next, m.prev, k)
    d.fire(m.effective())
    refused(_lib.CG_EINVAL, d.upcoming_copy, 20)
    d.free()


# arguments
def test_arguments(eng):
    d, nx, pv = delay_table(eng, np.arange(1, 301), T0)
    for k in (0, -1, KMAX + 1):
        refused(_lib.CG_EINVAL, d.upcoming_count, k)
    refused(_lib.CG_EINVAL, d.upcoming_copy, 1)  # no list yet
    check(d, nx, pv, KMAX)
    assert d.upcoming_count(200) == (200, 300)
    buf = np.zeros(200, dtype=np.int32)
    f = _lib.lib().cg_dispatcher_upcoming_copy
    assert f(d._h, buf.ctypes.data, None, None, 199) == _lib.CG_ECAPACITY and "200" in _lib.last_error()
    assert f(d._h, buf.ctypes.data, None, None, 200) == 0 and buf.tolist() == list(range(200))
    assert f(d._h, None, None, None, 0) == 0
    p = d.upcoming_device()
    assert p[0] and p[1] and p[2] and p[3] == 200
    # per node: unbound
    refused(_lib.CG_EINVAL, d.upcoming_count, 5, None, 0)
    d.free()


# 7. it disturbs nothing
def _rules(R, N, seed):
    """Node 0 on every rule, node N-1 on none, rule R // 2 on no node, every
    other rule on node 0 and 1-3 more nodes; every rule its own job."""
    from cronsun_amd.engine import RulesIn
    rng = np.random.default_rng(seed)
    lists = []
    for r in range(R):
        if r == R // 2:
            lists.append(np.zeros(0, np.int32))
            continue
        k = int(rng.integers(1, 4))
        lists.append(np.concatenate([[0], rng.choice(np.arange(1, N - 1), k, replace=False)]).astype(np.int32))
    nid_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    zero = np.zeros(R + 1, dtype=np.int64)
    return RulesIn(N, 0, R, R, group_off=np.zeros(1, np.int64), group_nodes=np.zeros(0, np.int32),
                   group_exists=np.zeros(0, np.uint8), rule_job=np.arange(R, dtype=np.int32),
                   nid_off=nid_off, nids=np.concatenate(lists), gid_off=zero, gids=np.zeros(0, np.int32),
                   ex_off=zero, ex=np.zeros(0, np.int32), job_pause=np.zeros(R, np.uint8))


def test_disturbs_nothing(eng):
    rng = np.random.default_rng(7)
    R, N = 900, 7
    delays = rng.choice([10, 10, 25, 40], R)
    rin = _rules(R, N, 70)
    drules = eng.upload_rules(rin)
    a, nx, pv = delay_table(eng, delays, T0)
    b, _, _ = delay_table(eng, delays, T0)
    for x in (a, b):
        x.bind_rules(drules, _lib.EXCLUDE_NONE)
    due_a, _ = a.fire(T0 + 10)
    due_b, _ = b.fire(T0 + 10)
    nx = np.where(delays == 10, T0 + 20, nx)
    pv = np.where(delays == 10, T0 + 10, pv)
    check(a, nx, pv, 500)
    check(a, nx, pv, 50, node=3, rows=node_rows(*eng.rule_nodes(rin), N)[3])
    got = np.empty(len(due_a), dtype=np.int32)
    assert _lib.lib().cg_dispatcher_due(a._h, 0, len(due_a), got.ctypes.data) == 0
    assert np.array_equal(got, due_a) and np.array_equal(due_a, due_b) and len(due_a) > 100
    off_a, sl_a = a.fanout()
    off_b, sl_b = b.fanout()
    assert np.array_equal(off_a, off_b) and np.array_equal(sl_a, sl_b) and len(sl_a) > len(due_a)
    # and the list is still readable behind the fan-out
    assert a.upcoming_device()[3] == 50
    sa, sb = a.snapshot(), b.snapshot()
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    for x in (a, b, drules):
        x.free()


# 8. per node
def test_per_node(eng):
    rng = np.random.default_rng(8)
    R, N = 5000, 7  # node 0's row is longer than a tile
    delays = rng.integers(1, 2000, R)
    rin = _rules(R, N, 80)
    w = World(rin)
    drules = eng.upload_rules(rin)
    d, nx, pv = delay_table(eng, delays, T0)
    d.bind_rules(drules, _lib.EXCLUDE_NONE)

    def all_nodes(rows, nx, pv, what):
        assert len(rows[0]) >= R - 2 and len(rows[N - 1]) in (0, 1)
        for node in range(N):
            for k in (1, 30, len(rows[node]) + 1, KMAX):
                check(d, nx, pv, k, rows=rows[node], node=node, what=what)
            check(d, nx, pv, 400, until=T0 + 700, rows=rows[node], node=node, what=what)
        check(d, nx, pv, KMAX, what=what)  # and cluster-wide

    rows = node_rows(*eng.rule_nodes(rin), N)
    assert len(rows[0]) == R - 1 and len(rows[N - 1]) == 0
    all_nodes(rows, nx, pv, "bound")
    for node in (-1, N, N + 100):
        refused(_lib.CG_EINVAL, d.upcoming_count, 5, None, node)
    # after a wake, so Prev is set
    due, _ = d.fire(d.effective)
    nx[due], pv[due] = nx[due] + delays[due], nx[due]
    # slots past the bound rule count are on no node
    d.set([R, R + 2], [cron.Every(10**9), cron.Every(2 * 10**9)], T0 + 1)
    nx = np.concatenate([nx, [T0 + 2, Z, T0 + 3]])
    pv = np.concatenate([pv, [Z, Z, Z]])
    all_nodes(rows, nx, pv, "past the count")
    assert d.upcoming_total == R + 2  # cluster-wide they are listed
    # one patch: slot R joins nodes 0 and 3, rule 9 leaves every node, rule 5
    # moves to the node that had nothing
    w.add_job([([0, 3], [], [], 0)])
    w.nids[9] = np.zeros(0, np.int32)
    w.nids[5] = np.array([N - 1], dtype=np.int32)
    patch, slots = w.patch([5, 9, R])
    d.upcoming_count(5, None, 0)
    dp = eng.upload_rules(patch)
    d.patch_rules(dp, slots)
    refused(_lib.CG_EINVAL, d.upcoming_copy, 5)  # the list described the old join
    rows = node_rows(*eng.rule_nodes(w.pack()), N)
    assert rows[N - 1].tolist() == [5] and R in rows[3] and 9 not in rows[0]
    all_nodes(rows, nx, pv, "patched")
    for x in (d, drules, dp):
        x.free()


# 9. past one block of tiles, 10. determinism
N_BIG = 263 * TILE + 5  # the per-tile counts are longer than one 256-thread block covers


@pytest.fixture(scope="module")
def big(eng):
    rng = np.random.default_rng(9)
    delays = rng.integers(1, 30 * DAY + 1, N_BIG)
    d, nx, pv = delay_table(eng, delays, T0)
    removed = rng.choice(N_BIG, N_BIG // 20, replace=False)
    d.remove(removed)
    nx[removed] = Z
    yield d, nx, pv
    d.free()


@pytest.mark.parametrize("k", [1, 100, KMAX])
def test_past_one_block_of_tiles(big, k):
    d, nx, pv = big
    p40 = int(np.percentile(nx[nx != Z], 40))
    check(d, nx, pv, k)
    check(d, nx, pv, k, until=p40)
    assert d.upcoming_total == int(((nx != Z) & (nx <= p40)).sum())


def test_deterministic(big):
    d, nx, pv = big
    p40 = int(np.percentile(nx[nx != Z], 40))
    runs = []
    for _ in range(2):
        out = []
        for k in (1, 100, KMAX):
            for until in (None, p40):
                out.append(b"".join(x.tobytes() for x in d.upcoming(k, until)))
        runs.append(out)
    assert runs[0] == runs[1] and len(runs[0][4]) == KMAX * 20
