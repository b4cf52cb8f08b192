"""tests/upcoming_model.py pinned on the CPU before it judges the kernels: to a
brute-force Python sorted() on seeded small tables (duplicates, zero times, the
no-progress value, an `until`, a node's row), and to
dispatch_model.DispatchModel: with until = effective and k = n the slots are
the next fire's due list."""
import numpy as np
import pytest

import oracle_lib as O
from common import oracle_parse_all, oracle_zone, random_spec
from dispatch_model import DispatchModel
from upcoming_model import NO_PROGRESS, ZERO_TIME, node_rows, upcoming

T0 = 1767225600


def brute(next, prev, k, until, rows):
    slots = range(len(next)) if rows is None else [int(s) for s in rows if 0 <= int(s) < len(next)]
    firing = [(int(next[s]), s) for s in slots
              if int(next[s]) not in (ZERO_TIME, NO_PROGRESS) and (until is None or int(next[s]) <= until)]
    out = sorted(firing)[:k]
    return ([s for _, s in out], [t for t, _ in out], [int(prev[s]) for _, s in out], len(firing))


def _table(rng, n):
    nx = T0 + rng.integers(-50, 50, n)  # few distinct values: many ties
    nx[rng.random(n) < 0.15] = ZERO_TIME
    nx[rng.random(n) < 0.1] = NO_PROGRESS
    pv = np.where(rng.random(n) < 0.5, ZERO_TIME, T0 - rng.integers(1, 1000, n))
    return nx.astype(np.int64), pv.astype(np.int64)


@pytest.mark.parametrize("seed", range(8))
def test_model_vs_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 200))
    nx, pv = _table(rng, n)
    assert n < 20 or ((nx == ZERO_TIME).any() and (nx == NO_PROGRESS).any())
    rows = np.sort(rng.choice(n + 3, max(n // 3, 1), replace=False))  # some slots past the table
    for until in (None, T0 - 51, T0 - 10, T0, T0 + 49):
        for r in (None, rows, np.zeros(0, np.int64)):
            for k in (1, 2, n // 2 + 1, n, n + 5):
                s, a, b, tot = upcoming(nx, pv, k, until, r)
                es, ea, eb, etot = brute(nx, pv, k, until, r)
                assert (s.tolist(), a.tolist(), b.tolist(), tot) == (es, ea, eb, etot), (until, k)
                assert s.dtype == np.int32 and a.dtype == b.dtype == np.int64


def test_model_vs_dispatch_model():
    """After every wake of a mixed table (specs + delays): until = effective
    and k = n give the next fire's due list, and the unbounded list is the
    whole firing table in (Next, slot) order."""
    rng = np.random.default_rng(11)
    n = 300
    specs = [random_spec(rng) for _ in range(n // 2)] + ["0 0 0 30 Feb ?"]
    sched = list(oracle_parse_all(specs)) + [int(x) for x in rng.integers(1, 900, n - len(specs))]
    m = DispatchModel(oracle_zone("UTC"), sched)
    m.start(T0)
    m.remove([3, 200])
    for w in range(6):
        e = m.effective()
        s, a, b, tot = upcoming(m.next, m.prev, n, until=e)
        s_all, a_all, _, tot_all = upcoming(m.next, m.prev, n)
        assert tot_all == int((m.next != ZERO_TIME).sum()) == len(s_all)
        assert np.all(np.diff(a_all) >= 0) and a_all[0] == e
        due, _ = m.fire(e + int(rng.choice([0, 1, 61])))
        assert np.array_equal(s, due) and tot == len(due) and np.all(a == e), w
        assert np.array_equal(s_all[:tot], due)
    assert (m.prev != ZERO_TIME).any()


def test_node_rows():
    rn_off = np.array([0, 2, 2, 5, 6])
    rn_nodes = np.array([1, 0, 2, 0, 1, 1, 99])  # (capacity past nnz is ignored)
    rows = node_rows(rn_off, rn_nodes, 4)
    assert [r.tolist() for r in rows] == [[0, 2], [0, 2, 3], [2], []]
    assert O.ZERO_TIME == ZERO_TIME
