"""The first k entries of Cron.Entries() (node/cron/cron.go:166-174: the entry
list in sort.Sort(byTime) order, cron.go:62-79) over the firing entries of a
dispatcher table, as numpy array math.

A firing entry has a Next that is neither the zero time nor the no-progress
value; byTime sorts every other entry last.  Equal Next values are listed in
ascending slot order: one of the orders the reference's unstable sort may
give, and the order of the due list.

tests/test_upcoming_model.py pins this file on the CPU (a brute-force sorted()
and dispatch_model.DispatchModel); the GPU tests then hold
cg_dispatcher_upcoming* to it.  No GPU import here.
"""
import numpy as np

ZERO_TIME = -62135596800         # Go time.Time{}.Unix()
NO_PROGRESS = -(1 << 63) + 1     # CG_NO_PROGRESS_TIME
NO_BOUND = (1 << 63) - 1


def upcoming(next, prev, k, until=None, rows=None):
    """next, prev: the table's columns (int64 per slot).  rows: a node's slot
    list (ascending), None for every slot; slots outside the table are on no
    node.  -> (slots int32, next, prev, n_total): the first min(k, n_total)
    firing entries with Next <= until by (Next, slot), and how many there are."""
    next = np.asarray(next, dtype=np.int64)
    prev = np.asarray(prev, dtype=np.int64)
    until = NO_BOUND if until is None else int(until)
    slot = np.arange(len(next), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    slot = slot[(slot >= 0) & (slot < len(next))]
    nx = next[slot]
    keep = (nx != ZERO_TIME) & (nx != NO_PROGRESS) & (nx <= until)
    slot, nx = slot[keep], nx[keep]
    order = np.lexsort((slot, nx))[:max(int(k), 0)]
    s = slot[order]
    return s.astype(np.int32), next[s], prev[s], int(keep.sum())


def node_rows(rn_off, rn_nodes, n_nodes):
    """The rule -> nodes CSR transposed: per node its rules, ascending."""
    rn_off = np.asarray(rn_off, dtype=np.int64)
    rule = np.repeat(np.arange(len(rn_off) - 1, dtype=np.int64), np.diff(rn_off))
    node = np.asarray(rn_nodes, dtype=np.int64)[:len(rule)]
    order = np.lexsort((rule, node))
    bounds = np.searchsorted(node[order], np.arange(n_nodes + 1))
    return [rule[order][bounds[n]:bounds[n + 1]] for n in range(n_nodes)]
