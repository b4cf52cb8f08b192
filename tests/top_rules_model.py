"""Host model of the top rules of a profile bucket (cg_profile_top_rules_*).

Plain numpy, no call into the library or the oracle.  Row n has the candidate
rules lists_rule[lists_off[n]:lists_off[n+1]] and ranks column buckets[n] of
the rule matrix: its contributors are the candidates with a cell > 0, its top
list the contributors ordered by (count descending, rule index ascending) and
cut to k.  test_top_rules_model.py pins it to a brute-force Python sort; the
GPU tests hold the kernels to it.
"""
import numpy as np


def full_order(rule_matrix, rules, bucket):
    """(rule, count) of one row's contributors in the order of the definition:
    a stable lexsort by (-count, rule) over the non-zero candidates."""
    rules = np.asarray(rules, dtype=np.int64)
    cells = rule_matrix[rules, bucket].astype(np.int64) if len(rules) else np.zeros(0, dtype=np.int64)
    keep = cells > 0
    rules, cells = rules[keep], cells[keep]
    order = np.lexsort((rules, -cells))
    return rules[order], cells[order]


def top_rules(rule_matrix, lists_off, lists_rule, buckets, k):
    """(rule int32 [N, k] padded -1, count int32 [N, k] padded 0, n_listed
    int32 [N], n_contrib int32 [N], bucket int32 [N])."""
    N = len(lists_off) - 1
    rule = np.full((N, k), -1, dtype=np.int32)
    count = np.zeros((N, k), dtype=np.int32)
    n_listed = np.zeros(N, dtype=np.int32)
    n_contrib = np.zeros(N, dtype=np.int32)
    for n in range(N):
        r, c = full_order(rule_matrix, lists_rule[lists_off[n]:lists_off[n + 1]], int(buckets[n]))
        m = min(k, len(r))
        rule[n, :m], count[n, :m] = r[:m], c[:m]
        n_listed[n], n_contrib[n] = m, len(r)
    return rule, count, n_listed, n_contrib, np.asarray(buckets, dtype=np.int32).copy()


def cluster_lists(R):
    """The one cluster-wide row: all R rules, each once."""
    return np.array([0, R], dtype=np.int64), np.arange(R, dtype=np.int32)


def tie_at_cut(rule_matrix, lists_off, lists_rule, buckets, k):
    """Rows whose full order has equal cells at positions k-1 and k: the cut
    falls inside a run of equal counts, so the rule index decides."""
    rows = []
    for n in range(len(lists_off) - 1):
        _, c = full_order(rule_matrix, lists_rule[lists_off[n]:lists_off[n + 1]], int(buckets[n]))
        if len(c) > k and c[k - 1] == c[k]:
            rows.append(n)
    return rows


COLUMNS = ("rule", "count", "n_listed", "n_contrib", "bucket")


def same(what, got, exp):
    """Exact equality of two five-column results; names the first differing
    (row, position)."""
    for name, g, e in zip(COLUMNS, got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        if not np.array_equal(g, e):
            at = [int(x[0]) for x in np.nonzero(g != e)]
            where = f"row {at[0]} position {at[1]}" if g.ndim == 2 else f"row {at[0]}"
            raise AssertionError(f"{what}: {name}: {where}: {int(g[tuple(at)])} vs {int(e[tuple(at)])}")
