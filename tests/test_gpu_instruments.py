"""The device instruments every large-scale check ends in -- cg_checksum_device
(k_checksum), cg_count_value_device (k_count_eq), cg_fill_device,
cg_fill_rate_device (k_fill_stream), cg_node_checksum_enqueue
(k_node_checksums), cg_node_counts_to_device (k_node_counts) and
cg_node_csr_place (k_node_place) -- against host math: the checksums against
tests/instruments_ref.py (written from the header's definition, checked on
the CPU in tests/test_instruments_ref.py), the counts, fills and placements
against numpy.  Every comparison is exact.  The shapes are the kernels' edges
(wave, block, one block's eight iterations, the grid cap, the unrolled loops'
bounds), not the workload's."""
import numpy as np
import pytest

import instruments_ref as R
from cronsun_amd import _lib, cron, synth
from instruments_ref import INT32_MAX, INT32_MIN, INT64_MAX, INT64_MIN, M64

pytestmark = pytest.mark.gpu

# wave, block and one-block-of-8-iterations edges of grid_for(n, 2048, 8192)
LADDER = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 100_003]
PAST_GRID_CAP = 8192 * 2048 + 2049
FIRSTS = [0, (1 << 31) - 3, (1 << 32) - 3, 1 << 40, INT64_MAX - 2, -5]
ADDS = [0, 1, -1, INT64_MAX]
NP_T = {8: np.int64, 4: np.int32}
LO = {8: INT64_MIN, 4: INT32_MIN}
HI = {8: INT64_MAX, 4: INT32_MAX}
BIG = (1 << 32) + 5


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda", 0)
    torch.zeros(1, device=d)  # torch's context first, the library's after it
    torch.cuda.synchronize(d)
    return d


@pytest.fixture(scope="module")
def eng(dev):
    from cronsun_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def up(dev, a):
    """A host array as a device tensor, complete before the library reads it."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    torch.cuda.synchronize(dev)
    return t


def code_of(fn, *args, **kw):
    with pytest.raises(_lib.CgError) as err:
        fn(*args, **kw)
    return err.value.code


def values(n, eb, seed):
    """Seeded values over the whole range of the type, its extremes at the
    first and last position and at 2047 and 2048 (where n reaches them)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(LO[eb], HI[eb], n, dtype=NP_T[eb], endpoint=True)
    for pos, x in ((2047, -1), (2048, 0), (0, LO[eb]), (n - 1, HI[eb])):
        if 0 <= pos < n:
            v[pos] = x
    return v


# ------------------------------------------------------------ 1. checksum
@pytest.mark.parametrize("n", LADDER)
@pytest.mark.parametrize("eb", [8, 4])
def test_checksum_vs_ref(eng, dev, eb, n):
    """cg_checksum_device against the reference at every first_index and add
    (wrap-around mod 2^64 included), at a pointer an odd number of elements
    into the tensor, twice in a row, and split at cuts (the parts add up)."""
    v = values(n, eb, 100 + n)
    d = up(dev, v)
    for first in FIRSTS:
        for add in ADDS:
            got = eng.checksum(d.data_ptr(), n, eb, first_index=first, add=add)
            assert got == R.checksum_ref_np(v, eb, first, add), (first, add)
    if n <= 257:  # the definition itself, in Python integers
        assert eng.checksum(d.data_ptr(), n, eb, -5, -1) == R.checksum_ref(v.tolist(), eb, -5, -1)
    # the accumulator is zeroed per call
    exp = R.checksum_ref_np(v, eb, 7, 1)
    assert eng.checksum(d.data_ptr(), n, eb, 7, 1) == exp
    assert eng.checksum(d.data_ptr(), n, eb, 7, 1) == exp
    # 8-byte (int64) / 4-byte (int32) alignment: 1 and 3 elements into a tensor
    # whose other elements would change the sum if they were read
    for skip in (1, 3):
        buf = np.full(n + 6, 0x5A5A5A5A, dtype=NP_T[eb])
        buf[skip:skip + n] = v
        db = up(dev, buf)
        assert eng.checksum(db.data_ptr() + skip * eb, n, eb, (1 << 32) - 3, -1) == \
            R.checksum_ref_np(v, eb, (1 << 32) - 3, -1), skip
    # device additivity: [0, cut) at first_index base plus [cut, n) at base + cut
    for base in (0, (1 << 32) - 3):
        whole = R.checksum_ref_np(v, eb, base, 0)
        for cut in sorted({1, 64, 2048, n - 1}):
            if not 0 < cut < n:
                continue
            a = eng.checksum(d.data_ptr(), cut, eb, base)
            b = eng.checksum(d.data_ptr() + cut * eb, n - cut, eb, base + cut)
            assert a == R.checksum_ref_np(v[:cut], eb, base) and b == R.checksum_ref_np(v[cut:], eb, base + cut), cut
            assert (a + b) & M64 == whole, cut


def test_checksum_past_the_grid_cap(eng, dev):
    """8192 blocks and more than one grid stride per thread -- the only regime
    the config-scale parity checks run in (int64, 134 MB)."""
    n = PAST_GRID_CAP
    v = values(n, 8, 5)
    d = up(dev, v)
    for first, add in ((0, 0), ((1 << 32) - 3, -1)):
        assert eng.checksum(d.data_ptr(), n, 8, first, add) == R.checksum_ref_np(v, 8, first, add), (first, add)


@pytest.mark.parametrize("eb", [8, 4])
def test_checksum_sensitivity(eng, dev, eb):
    """Neighbours swapped, bit 0 and a high bit (40; the sign bit for int32)
    of one element flipped, the last element changed: the reference of the
    altered array differs from the original's, and the device agrees with it."""
    n = 4097
    v = values(n, eb, 9)
    base = R.checksum_ref_np(v, eb, 3, 0)
    assert eng.checksum(up(dev, v).data_ptr(), n, eb, 3) == base
    high = 40 if eb == 8 else 31
    alts = []
    for i in (0, 63, 2047, n - 2):
        assert v[i] != v[i + 1]
        w = v.copy()
        w[[i, i + 1]] = w[[i + 1, i]]
        alts.append(("swap", i, w))
    for i in (0, 255, 2048, n - 1):
        for bit in (0, high):
            w = v.copy()
            w[i:i + 1].view(np.uint64 if eb == 8 else np.uint32)[0] ^= (1 << bit)
            alts.append((f"bit{bit}", i, w))
    w = v.copy()
    w[n - 1] -= 1
    alts.append(("last", n - 1, w))
    for what, i, w in alts:
        exp = R.checksum_ref_np(w, eb, 3, 0)
        assert exp != base, (what, i)
        assert eng.checksum(up(dev, w).data_ptr(), n, eb, 3) == exp, (what, i)


def test_checksum_bad_arguments(eng, dev):
    d = up(dev, np.arange(8, dtype=np.int64))
    assert code_of(eng.checksum, d.data_ptr(), 8, 2) == _lib.CG_EINVAL
    assert code_of(eng.checksum, d.data_ptr(), -1, 8) == _lib.CG_EINVAL
    assert code_of(eng.checksum, 0, 8, 8) == _lib.CG_EINVAL
    assert eng.checksum(0, 0, 8) == 0  # nothing to read
    assert eng.checksum(d.data_ptr(), 8, 8) == R.checksum_ref(range(8), 8)


# --------------------------------------------------------- 2. count_value
@pytest.mark.parametrize("n", LADDER)
@pytest.mark.parametrize("eb", [8, 4])
def test_count_value_vs_numpy(eng, dev, eb, n):
    """cg_count_value_device against np.count_nonzero: -1, 0, the type's
    minimum and 5 planted at block edges among other values; in int64 arrays
    2^32 + 5 beside 5 (neither counts as the other); in int32 arrays a value
    outside the int32 range equals no element."""
    rng = np.random.default_rng(200 + n)
    pool = [-1, 0, LO[eb], 5, 6, -2, HI[eb]] + ([BIG, BIG + 1, INT32_MIN, 5 - (1 << 32)] if eb == 8 else [])
    v = np.array(pool, dtype=NP_T[eb])[rng.integers(0, len(pool), n)]
    edges = sorted({p for p in (0, 1, 62, 63, 64, 254, 255, 256, 2046, 2047, 2048, 4095, 4096, n - 2, n - 1)
                    if 0 <= p < n})
    for k, p in enumerate(edges):
        v[p] = (-1, 0, LO[eb], 5)[k % 4] if eb == 4 else (-1, 0, LO[eb], 5, BIG)[k % 5]
    d = up(dev, v)
    v64 = v.astype(np.int64)
    asked = [-1, 0, INT64_MIN, INT32_MIN, 5, BIG, 6, 7, -(1 << 31) - 1, 5 - (1 << 32), INT64_MAX, INT32_MAX]
    for x in asked:
        assert eng.count_value(d.data_ptr(), n, eb, x) == int(np.count_nonzero(v64 == np.int64(x))), x
    if eb == 4:  # no int32 element equals these, whatever their low 32 bits
        for x in (BIG, -(1 << 31) - 1, 5 - (1 << 32), (1 << 32) - 1, INT64_MIN, 1 << 32):
            assert eng.count_value(d.data_ptr(), n, eb, x) == 0, x
    if n >= 63:  # at least four planted edges: a -1 and a 5 among them
        assert eng.count_value(d.data_ptr(), n, eb, 5) > 0 and eng.count_value(d.data_ptr(), n, eb, -1) > 0
    # a pointer one element into the tensor
    if n >= 1:
        assert eng.count_value(d.data_ptr() + eb, n - 1, eb, 5) == int(np.count_nonzero(v64[1:] == 5))


@pytest.mark.parametrize("eb", [8, 4])
def test_count_of_poison_after_fill(eng, dev, eb):
    """After cg_fill_device(..., 0xFF) every element counts as -1 (what the
    writer tests and the benchmark's "nothing left unwritten" rest on); one
    element written over takes one off the count."""
    import torch
    for n in (1, 255, 2049, 100_003):
        t = torch.zeros(n, dtype=torch.int64 if eb == 8 else torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        assert eng.count_value(t.data_ptr(), n, eb, -1) == 0
        eng.fill(t.data_ptr(), n * eb, 0xFF)
        assert eng.count_value(t.data_ptr(), n, eb, -1) == n
        assert eng.count_value(t.data_ptr(), n, eb, 0) == 0
        assert (t.cpu().numpy() == -1).all()
        t[n - 1] = 3
        torch.cuda.synchronize(dev)
        assert eng.count_value(t.data_ptr(), n, eb, -1) == n - 1


def test_count_value_bad_arguments(eng, dev):
    d = up(dev, np.arange(8, dtype=np.int64))
    assert code_of(eng.count_value, d.data_ptr(), 8, 2, 0) == _lib.CG_EINVAL
    assert code_of(eng.count_value, d.data_ptr(), -1, 8, 0) == _lib.CG_EINVAL
    assert code_of(eng.count_value, 0, 8, 8, 0) == _lib.CG_EINVAL
    assert eng.count_value(0, 0, 8, 0) == 0


# ---------------------------------------------------------------- 3. fill
@pytest.mark.parametrize("nbytes", [0, 1, 7, 8, 4093])
def test_fill_changes_exactly_the_requested_bytes(eng, dev, nbytes):
    """cg_fill_device from 3 bytes into a tensor holding another byte value:
    the requested bytes change, the bytes on either side keep theirs."""
    for old, new in ((0xA5, 0x3C), (0x00, 0xFF)):
        host = np.full(nbytes + 64, old, dtype=np.uint8)
        t = up(dev, host)
        eng.fill(t.data_ptr() + 3, nbytes, new)
        host[3:3 + nbytes] = new
        assert np.array_equal(t.cpu().numpy(), host)
    assert code_of(eng.fill, t.data_ptr(), -1, 0) == _lib.CG_EINVAL
    assert code_of(eng.fill, 0, 8, 0) == _lib.CG_EINVAL
    eng.fill(0, 0, 0)  # nothing to write


# ----------------------------------------------------------- 4. fill rate
@pytest.mark.parametrize("n16", [1, 255, 1025])
def test_fill_rate_stays_inside_its_bytes(eng, dev, n16):
    """cg_fill_rate_device over 16 * n16 bytes inside a larger poisoned
    tensor: the words before and after keep the poison, the three times are
    positive.  The buffer's final contents are those of the last fill, the
    memset (0x5E bytes), which covers whatever k_fill_stream wrote: this test
    can catch an overrun of k_fill_stream, not a gap in its coverage."""
    nbytes = 16 * n16
    host = np.full(32 + nbytes + 4096, 0xA5, dtype=np.uint8)
    t = up(dev, host)
    ms = eng.fill_rates(t.data_ptr() + 32, nbytes, reps=2)
    assert set(ms) == {"fill_stream_nt", "fill_stream_plain", "hipMemsetAsync"}
    assert all(x > 0 for x in ms.values()), ms
    host[32:32 + nbytes] = 0x5E
    assert np.array_equal(t.cpu().numpy(), host)
    for bad in (nbytes - 1, nbytes + 8, 0):
        assert code_of(eng.fill_rates, t.data_ptr() + 32, bad, 2) == _lib.CG_EINVAL
    assert np.array_equal(t.cpu().numpy(), host)


# ---------------------------------------- 5. / 6. per-node checksums, counts
SENTINEL = 0x5555555555555555
MODE = _lib.EXCLUDE_NONE


class World:
    """test_gpu_comm.py's small world (500 multi-rule jobs, config 2's spec
    mix, one hour: a little over 10^4 node events) plus three nodes no rule
    names, whose lists are empty."""

    def __init__(self):
        self.rin = synth.multi_rule_jobs(500, seed=77, key_choices=2)
        self.rin.n_nodes += 3
        self.N = self.rin.n_nodes
        self.specs = synth.spec_mix(self.rin.n_rules, seed=78, mix=synth.MIX_CONFIG2)
        self.scheds = [cron.Parse(s) for s in self.specs]
        self.arr, status = cron.parse_batch(self.specs)
        assert (status == 0).all()
        self.t0 = synth.T0_2026 + 5 * 86400
        self.utc = cron.UTC()
        self.ask = np.array(list(range(self.N)) + [-1, self.N, self.N + 7], dtype=np.int32)


@pytest.fixture(scope="module")
def world():
    return World()


def expected_rows(world, node_off, time, rule):
    """The reference's (time, rule) checksum pair of every asked node's list;
    (0, 0) for the entries that name no node."""
    exp = np.zeros((len(world.ask), 2), dtype=np.uint64)
    for i, n in enumerate(world.ask):
        if 0 <= n < world.N:
            a, b = int(node_off[n]), int(node_off[n + 1])
            exp[i] = R.node_list_checksum_ref(time[a:b].tolist(), rule[a:b].tolist())
    return exp


def out_rows(dev, rows, k):
    import torch
    t = torch.full((rows, 2 * k), SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    return t


def as_pairs(t):
    return t.cpu().numpy().view(np.uint64).reshape(t.shape[0], -1, 2)


@pytest.mark.parametrize("order", [_lib.NODE_ORDER_RULE, _lib.NODE_ORDER_TIME])
def test_node_checksums_and_counts_of_a_synchronous_result(dev, world, order):
    """cg_node_checksum_enqueue after a synchronous per-node call: every node
    plus the entries -1, N and N + 7 against the reference over the host copy
    of the same result (out-of-range entries and empty nodes give (0, 0));
    cg_node_counts_to_device equals the differences of the node offsets;
    k = 0 is accepted."""
    import torch
    from cronsun_amd.engine import Engine
    ask = up(dev, world.ask)
    k = len(world.ask)
    out = out_rows(dev, 1, k)
    counts = torch.full((world.N + 2,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    e = Engine(0)
    try:
        e.set_node_order(order)
        node_off, time, rule = e.expand_per_node(world.scheds, None, world.t0, world.t0 + 3600, world.rin, MODE)
        E = int(node_off[-1])
        assert E > 10000 and len(time) == E
        lens = np.diff(node_off)
        assert (lens[-3:] == 0).all() and (lens > 256).any() and (node_off[:-4] > 0).any()
        e.node_checksum_enqueue(ask.data_ptr(), k, out.data_ptr())
        e.node_checksum_enqueue(0, 0, 0)  # k = 0: nothing to do
        e.sync()
        got = as_pairs(out)[0]
        exp = expected_rows(world, node_off, time, rule)
        assert np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0]
        assert (got[-3:] == 0).all() and (got[world.N - 3:world.N] == 0).all()
        assert (got[:world.N - 3][lens[:-3] > 0] != 0).all()
        # a repeated node, another order of the entries
        sub = np.array([5, 5, world.N - 1, 0, -1, 5], dtype=np.int32)
        out2 = out_rows(dev, 1, len(sub))
        e.node_checksum_enqueue(up(dev, sub).data_ptr(), len(sub), out2.data_ptr())
        e.sync()
        pos = [int(np.nonzero(world.ask == n)[0][0]) for n in sub]
        assert np.array_equal(as_pairs(out2)[0], exp[pos])
        # 6. the counts the ranks all-gather
        e.node_counts_to_device(counts.data_ptr() + 8)
        c = counts.cpu().numpy()
        assert c[0] == -7 and c[-1] == -7 and np.array_equal(c[1:-1], lens)
    finally:
        e.close()


@pytest.mark.parametrize("order", [_lib.NODE_ORDER_RULE, _lib.NODE_ORDER_TIME])
def test_node_checksums_belong_to_the_window_they_follow(dev, world, order):
    """Two different pipelined windows, cg_node_checksum_enqueue into its own
    row behind each, one wait: each row equals the reference over the
    synchronous result of its window, computed afterwards -- the checksum is of
    the window it was enqueued behind, although the second window has
    overwritten the first by the time of the wait (what bench.py's every-step
    verification relies on)."""
    from cronsun_amd.engine import Engine
    ask = up(dev, world.ask)
    k = len(world.ask)
    out = out_rows(dev, 2, k)
    t0 = world.t0
    wins = [(t0, t0 + 3600), (t0 + 1801, t0 + 1801 + 2400)]
    e = Engine(0)
    try:
        e.set_node_order(order)
        sp, dr = e.upload_c(world.arr, world.rin.n_rules), e.upload_rules(world.rin)
        e.expand_per_node_rules_device(sp, world.utc, t0, t0 + 4096, dr, MODE)  # sizes the outputs
        for i, (a, b) in enumerate(wins):
            e.expand_per_node_async(sp, world.utc, a, b, dr, MODE)
            e.node_checksum_enqueue(ask.data_ptr(), k, out[i].data_ptr())
        En_last = e.expand_per_node_wait()
        got = as_pairs(out)
        exps = []
        for i, (a, b) in enumerate(wins):
            En, _ = e.expand_per_node_rules_device(sp, world.utc, a, b, dr, MODE)
            node_off, time, rule = e.node_result(world.N, En)
            assert int(node_off[-1]) == En > 5000
            exps.append(expected_rows(world, node_off, time, rule))
            assert np.array_equal(got[i], exps[i]), (i, np.nonzero((got[i] != exps[i]).any(axis=1))[0])
        assert En_last == En
        assert not np.array_equal(exps[0], exps[1])
        dr.free()
        sp.free()
    finally:
        e.close()


@pytest.mark.parametrize("order", [_lib.NODE_ORDER_RULE, _lib.NODE_ORDER_TIME])
def test_node_checksums_of_a_window_past_the_capacity_are_zero(dev, world, order):
    """A 4096-s window past the output capacity a 300-s window sized: its row
    of checksums is all zeros (nothing is read), the wait returns
    CG_ECAPACITY, and a later good window's row checks out."""
    from cronsun_amd.engine import Engine
    ask = up(dev, world.ask)
    k = len(world.ask)
    out = out_rows(dev, 2, k)
    t0 = world.t0
    e = Engine(0)
    try:
        e.set_node_order(order)
        sp, dr = e.upload_c(world.arr, world.rin.n_rules), e.upload_rules(world.rin)
        Es, _ = e.expand_per_node_rules_device(sp, world.utc, t0, t0 + 300, dr, MODE)
        node_off, time, rule = e.node_result(world.N, Es)
        exp = expected_rows(world, node_off, time, rule)
        e.expand_per_node_async(sp, world.utc, t0, t0 + 4096, dr, MODE)
        e.node_checksum_enqueue(ask.data_ptr(), k, out[0].data_ptr())
        assert code_of(e.expand_per_node_wait) == _lib.CG_ECAPACITY
        assert (as_pairs(out)[0] == 0).all()
        e.expand_per_node_async(sp, world.utc, t0, t0 + 300, dr, MODE)
        e.node_checksum_enqueue(ask.data_ptr(), k, out[1].data_ptr())
        assert e.expand_per_node_wait() == Es
        got = as_pairs(out)
        assert (got[0] == 0).all()
        assert np.array_equal(got[1], exp) and (exp != 0).any()
        dr.free()
        sp.free()
    finally:
        e.close()


def test_node_checksum_without_a_per_node_result_is_refused(dev):
    from cronsun_amd.engine import Engine
    ask = up(dev, np.zeros(4, dtype=np.int32))
    out = out_rows(dev, 1, 4)
    e = Engine(0)
    try:
        assert code_of(e.node_checksum_enqueue, ask.data_ptr(), 4, out.data_ptr()) == _lib.CG_EINVAL
        assert code_of(e.node_checksum_enqueue, ask.data_ptr(), 0, out.data_ptr()) == _lib.CG_EINVAL
        assert code_of(e.node_checksum_enqueue, ask.data_ptr(), -1, out.data_ptr()) == _lib.CG_EINVAL
        e.sync()
    finally:
        e.close()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------- 7. CSR placement
# the edges of k_node_place's `i + 768 < b` unrolled loop and of its tail
PLACE_LENS = [0, 1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 1791, 1792, 2049]


@pytest.fixture(scope="module")
def place_case():
    """5000 hand-built node lists (more than twice the kernel's grid, so the
    node loop strides): the edge lengths at nodes spread over the whole range,
    its first and last nodes included, short random lists elsewhere; every
    node's destination a random gap after the previous node's."""
    rng = np.random.default_rng(42)
    N = 5000
    lens = rng.integers(0, 13, N)
    at = np.linspace(0, N - 1, len(PLACE_LENS)).astype(np.int64)
    lens[at] = rng.permutation(PLACE_LENS)
    src_off = np.zeros(N + 1, dtype=np.int64)
    src_off[1:] = np.cumsum(lens)
    E = int(src_off[-1])
    src_time = rng.integers(synth.T0_2026, synth.T0_2026 + 7 * 86400, E).astype(np.int64)
    src_rule = rng.integers(0, 10_000_000, E).astype(np.int32)
    gaps = rng.integers(0, 6, N)
    gaps[0] = 3
    gaps[at[1:]] = rng.integers(1, 6, len(at) - 1)  # a guard word right before every edge-length list
    dst_start = np.cumsum(gaps) + src_off[:-1]
    total = int(dst_start[-1] + lens[-1]) + 64
    return N, src_off, src_time, src_rule, dst_start.astype(np.int64), total


@pytest.mark.parametrize("rule_add", [0, 1000, -3])
def test_node_csr_place_vs_numpy(eng, dev, place_case, rule_add):
    """cg_node_csr_place into buffers pre-filled with -1: every placed event
    equals numpy's placement (rules shifted by rule_add), every gap word and
    the words past the end still hold -1."""
    import torch
    N, src_off, src_time, src_rule, dst_start, total = place_case
    exp_t = np.full(total, -1, dtype=np.int64)
    exp_r = np.full(total, -1, dtype=np.int32)
    for n in range(N):
        a, b, d = int(src_off[n]), int(src_off[n + 1]), int(dst_start[n])
        assert (exp_t[d:d + b - a] == -1).all()  # the hand-built destinations do not overlap
        exp_t[d:d + b - a] = src_time[a:b]
        exp_r[d:d + b - a] = src_rule[a:b] + rule_add
    assert np.count_nonzero(exp_t == -1) == total - int(src_off[-1])
    d_off, d_t, d_r, d_start = up(dev, src_off), up(dev, src_time), up(dev, src_rule), up(dev, dst_start)
    out_t = torch.full((total,), -1, dtype=torch.int64, device=dev)
    out_r = torch.full((total,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    eng.node_csr_place(0, 0, 0, 0, rule_add, 0, 0, 0)  # n_nodes = 0: accepted, nothing placed
    eng.node_csr_place(0, d_off.data_ptr(), d_t.data_ptr(), d_r.data_ptr(), rule_add, d_start.data_ptr(),
                       out_t.data_ptr(), out_r.data_ptr())
    assert (out_t.cpu().numpy() == -1).all() and (out_r.cpu().numpy() == -1).all()
    eng.node_csr_place(N, d_off.data_ptr(), d_t.data_ptr(), d_r.data_ptr(), rule_add, d_start.data_ptr(),
                       out_t.data_ptr(), out_r.data_ptr())
    got_t, got_r = out_t.cpu().numpy(), out_r.cpu().numpy()
    assert np.array_equal(got_t, exp_t), np.nonzero(got_t != exp_t)[0][:8]
    assert np.array_equal(got_r, exp_r), np.nonzero(got_r != exp_r)[0][:8]
    # the device's own judges agree with the host about the placed arrays
    assert eng.count_value(out_t.data_ptr(), total, 8, -1) == total - int(src_off[-1])
    assert eng.checksum(out_t.data_ptr(), total, 8) == R.checksum_ref_np(exp_t, 8)
    assert eng.checksum(out_r.data_ptr(), total, 4) == R.checksum_ref_np(exp_r, 4)
