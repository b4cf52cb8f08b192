"""Host model of the fire profile (cg_profile.hip): the rule matrix, its
column totals and the node matrix of a rule set that repeats a small base set.

Plain numpy, no call into the library or the oracle.  A large rule set is a
base set of K rules picked R times: rule r = base rule pick[r].  With `base`
the int32 [K, B] matrix of the base set (bin_fires over one oracle expansion),
every expectation at any R costs a gather or a K-wide integer product.
test_profile_model.py pins the model to the oracle's join and fire lists at
the sizes the oracle can walk; test_gpu_profile_scale.py then holds the
kernels to it on both sides of every chunk, tile and grid-cap edge.
"""
import numpy as np


def bin_fires(off, times, t0, w, B):
    """int32 [K, B] from a CSR of fire lists (off [K+1], times in (t0, ...]):
    a fire at t is in bucket (t - t0 - 1) // w; fires past t0 + B*w are
    dropped, so one expansion over the longest horizon serves every (w, B)
    inside it."""
    K = len(off) - 1
    rule = np.repeat(np.arange(K, dtype=np.int64), np.diff(off))
    b = (np.asarray(times, dtype=np.int64) - t0 - 1) // w
    keep = (b >= 0) & (b < B)
    return np.bincount(rule[keep] * B + b[keep], minlength=K * B).reshape(K, B).astype(np.int32)


def rule_matrix(base, pick):
    """int32 [R, B]: row r is the base row pick[r]."""
    return base[pick]


def totals(base, pick):
    """int64 [B]: the column sums of rule_matrix(base, pick)."""
    return np.bincount(pick, minlength=base.shape[0]).astype(np.int64) @ base.astype(np.int64)


def node_matrix(nt_off, nt_rule, rule_counts):
    """int64 [N, B]: per node the sum of its rules' rows (nt_off [N+1],
    nt_rule: the node-major join).  A running sum over the listed rows
    differenced at nt_off, so an empty node is a zero row."""
    B = rule_counts.shape[1]
    run = np.zeros((len(nt_rule) + 1, B), dtype=np.int64)
    np.cumsum(rule_counts[nt_rule], axis=0, dtype=np.int64, out=run[1:])
    return run[nt_off[1:]] - run[nt_off[:-1]]


def node_weights(nt_off, nt_rule, pick, K):
    """int64 [N, K]: W[n, k] = the pairs (n, r) of the join with pick[r] == k."""
    N = len(nt_off) - 1
    node = np.repeat(np.arange(N, dtype=np.int64), np.diff(nt_off))
    return np.bincount(node * K + pick[nt_rule], minlength=N * K).reshape(N, K)


def node_matrix_tiled(nt_off, nt_rule, pick, base):
    """node_matrix(nt_off, nt_rule, base[pick]) by linearity: W @ base, which
    never forms the [R, B] matrix."""
    return node_weights(nt_off, nt_rule, pick, base.shape[0]) @ base.astype(np.int64)


def make_pick(K, R, seed):
    """int64 [R] over [0, K) with pick[i] != pick[i+1] for all i and, for
    2R >= 3K, every value present: a row read one place off, skipped or
    counted twice is then a different base row."""
    rng = np.random.default_rng(seed)
    if K == 1:
        return np.zeros(R, dtype=np.int64)
    step = rng.integers(1, K, R)  # 1 .. K-1: never back onto the same value
    step[0] = rng.integers(0, K)
    pick = np.cumsum(step) % K
    if 2 * R >= 3 * K:
        missing = np.setdiff1d(np.arange(K), pick)
        cnt = np.bincount(pick, minlength=K)
        for m in missing.tolist():
            while True:
                i = int(rng.integers(1, R - 1))
                if cnt[pick[i]] > 1 and pick[i - 1] != m and pick[i + 1] != m:
                    cnt[pick[i]] -= 1
                    pick[i] = m
                    cnt[m] += 1
                    break
    return pick.astype(np.int64)
