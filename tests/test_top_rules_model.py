"""The host model of the top-rules calls (top_rules_model.py) against a
brute-force Python sort on hand-made matrices: ties at the cut, k greater
than the number of contributors, a zero row, one candidate."""
import numpy as np
import pytest

import top_rules_model as TM


def brute(matrix, off, rule, buckets, k):
    """sorted() over Python tuples, row by row."""
    rows = []
    for n in range(len(off) - 1):
        b = int(buckets[n])
        cand = [(int(matrix[r][b]), int(r)) for r in rule[off[n]:off[n + 1]]]
        full = sorted([(c, r) for c, r in cand if c > 0], key=lambda x: (-x[0], x[1]))
        top = full[:k]
        rows.append(([r for _, r in top] + [-1] * (k - len(top)), [c for c, _ in top] + [0] * (k - len(top)),
                     len(top), len(full), b))
    return tuple(np.array([row[i] for row in rows], dtype=np.int32).reshape((len(rows), k) if i < 2 else -1)
                 for i in range(5))


#            bucket 0  1  2
MATRIX = np.array([[5, 0, 1],   # rule 0
                   [3, 0, 1],   # 1
                   [3, 0, 0],   # 2
                   [0, 0, 1],   # 3
                   [3, 0, 7],   # 4
                   [9, 0, 1],   # 5
                   [3, 0, 1]],  # 6
                  dtype=np.int32)
# row 0: every rule; row 1: rules 6, 4, 2, 1 (not ascending: the order of the
# candidates must not matter); row 2: no rule; row 3: one candidate
OFF = np.array([0, 7, 11, 11, 12], dtype=np.int64)
RULE = np.array([0, 1, 2, 3, 4, 5, 6, 6, 4, 2, 1, 3], dtype=np.int32)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 64])
@pytest.mark.parametrize("buckets", [[0, 0, 0, 0], [2, 2, 2, 2], [1, 1, 1, 1], [0, 2, 1, 2]])
def test_model_equals_brute_force(buckets, k):
    TM.same(f"buckets {buckets} k {k}", TM.top_rules(MATRIX, OFF, RULE, buckets, k),
            brute(MATRIX, OFF, RULE, buckets, k))


def test_ties_at_the_cut_go_to_the_smaller_rule():
    """Bucket 0 of row 0 in full order: 5 (9), 0 (5), then rules 1, 2, 4, 6
    with 3 each.  k = 3 and k = 4 cut inside the run of equal counts."""
    rule, count, n_listed, n_contrib, bucket = TM.top_rules(MATRIX, OFF, RULE, [0, 0, 0, 0], 3)
    assert rule[0].tolist() == [5, 0, 1] and count[0].tolist() == [9, 5, 3]
    assert rule[1].tolist() == [1, 2, 4] and count[1].tolist() == [3, 3, 3]  # 6 loses to all three
    assert n_listed.tolist() == [3, 3, 0, 0] and n_contrib.tolist() == [6, 4, 0, 0]
    assert TM.top_rules(MATRIX, OFF, RULE, [0, 0, 0, 0], 4)[0][0].tolist() == [5, 0, 1, 2]
    assert TM.tie_at_cut(MATRIX, OFF, RULE, [0, 0, 0, 0], 3) == [0, 1]
    assert TM.tie_at_cut(MATRIX, OFF, RULE, [0, 0, 0, 0], 2) == [1]
    assert TM.tie_at_cut(MATRIX, OFF, RULE, [0, 0, 0, 0], 6) == []


def test_k_beyond_the_contributors_pads():
    rule, count, n_listed, n_contrib, bucket = TM.top_rules(MATRIX, OFF, RULE, [2, 2, 2, 2], 8)
    assert rule[0].tolist() == [4, 0, 1, 3, 5, 6, -1, -1] and count[0].tolist() == [7, 1, 1, 1, 1, 1, 0, 0]
    assert (n_listed[0], n_contrib[0]) == (6, 6)  # rule 2's cell is zero: never listed
    assert count[0].sum() == MATRIX[:, 2].sum()
    assert rule.dtype == count.dtype == n_listed.dtype == n_contrib.dtype == bucket.dtype == np.int32


def test_zero_row_and_zero_column_list_nothing():
    rule, count, n_listed, n_contrib, bucket = TM.top_rules(MATRIX, OFF, RULE, [1, 1, 0, 1], 4)
    assert (rule == -1).all() and not count.any() and not n_listed.any() and not n_contrib.any()
    assert bucket.tolist() == [1, 1, 0, 1]


def test_one_candidate():
    rule, count, n_listed, n_contrib, _ = TM.top_rules(MATRIX, OFF, RULE, [0, 0, 0, 2], 2)
    assert rule[3].tolist() == [3, -1] and count[3].tolist() == [1, 0] and (n_listed[3], n_contrib[3]) == (1, 1)
    rule, count, n_listed, n_contrib, _ = TM.top_rules(MATRIX, OFF, RULE, [0, 0, 0, 0], 2)  # ... with a zero cell
    assert rule[3].tolist() == [-1, -1] and (n_listed[3], n_contrib[3]) == (0, 0)


def test_cluster_row_and_same_names_the_first_difference():
    off, rule = TM.cluster_lists(7)
    got = TM.top_rules(MATRIX, off, rule, [0], 64)
    assert got[0][0, :7].tolist() == [5, 0, 1, 2, 4, 6, -1] and got[3].tolist() == [6]
    bad = tuple(x.copy() for x in got)
    bad[1][0, 2] += 1
    with pytest.raises(AssertionError, match=r"count: row 0 position 2: 4 vs 3"):
        TM.same("x", bad, got)
