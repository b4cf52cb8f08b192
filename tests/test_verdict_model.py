"""The fire-verdict model (verdict_model.py) pinned to hand-derived cases: each
expected byte below is worked out from the definition in
include/cronsun_gpu.h ("fire verdicts"), not from running the model."""
import numpy as np
import pytest

import verdict_model as VM
from lock_model import ALONE, COMMON, INTERVAL, LockStuck

D, S = VM.DROPPED, VM.SKIPPED


def csr(*lists):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, np.array([t for x in lists for t in x], dtype=np.int64)


def test_two_rules_same_second_rule_order_decides():
    """One unit, P = 1, d = 10 s: rules 0 and 1 both fire at 100.  Rule 0 is
    taken first and admitted; rule 1 finds one running and is dropped.  At 110
    the instance of 100 has ended (100 + 10 <= 110): rule 1's fire is admitted."""
    off, times = csr([100], [100, 110])
    v = VM.verdicts_from_lists(off, times, 0, 1000, admit=([10_000] * 2, [1, 1], [0, 0]))
    assert v.tolist() == [0, D, 0]
    # as units of their own nothing drops
    v = VM.verdicts_from_lists(off, times, 0, 1000, admit=([10_000] * 2, [1, 1], None))
    assert v.tolist() == [0, 0, 0]


def test_fire_at_the_second_an_instance_ends_is_admitted():
    """P = 1, 5000 ms: 10 admitted, 14 dropped (10 + 5 > 14), 15 admitted
    (10 * 1000 + 5000 > 15 * 1000 is false).  5001 ms rounds up to 6 s: 15
    dropped, 16 admitted."""
    off, times = csr([10, 14, 15, 16])
    assert VM.verdicts_from_lists(off, times, 0, 100, admit=([5000], [1], None)).tolist() == [0, D, 0, D]
    assert VM.verdicts_from_lists(off, times, 0, 100, admit=([5001], [1], None)).tolist() == [0, D, D, 0]


def test_zero_duration_and_no_limit_admit_everything():
    off, times = csr([1, 1 + 1, 3], [1, 2, 3])
    assert not VM.verdicts_from_lists(off, times, 0, 10, admit=([0] * 2, [1, 1], [4, 4])).any()
    assert not VM.verdicts_from_lists(off, times, 0, 10, admit=([10**6] * 2, [0, 0], [4, 4])).any()


def test_p_two_ring():
    """P = 2, d = 10: fires 1, 2, 3, 11, 12, 13.  1 and 2 admitted, 3 dropped;
    at 11 the run of 1 has ended: admitted (running {2, 11}); at 12 that of 2
    has ended: admitted (running {11, 12}); 13 dropped."""
    off, times = csr([1, 2, 3, 11, 12, 13])
    assert VM.verdicts_from_lists(off, times, 0, 20, admit=([10_000], [2], None)).tolist() == [0, 0, D, 0, 0, D]


def test_duration_is_clamped_to_the_horizon():
    """INT64_MAX ms over a horizon of 20 s: d = 20, the first fire is admitted
    and every later one of the horizon dropped."""
    off, times = csr([1, 20])
    assert VM.verdicts_from_lists(off, times, 0, 20, admit=([2**63 - 1], [1], None)).tolist() == [0, D]


def test_lock_interval_and_the_second_the_lease_ends():
    """INTERVAL, ttl 5 at every fire: 10 granted (free_at 15), 12 and 14
    skipped, 15 granted (t < free_at is false; free_at 20), 19 skipped, 20
    granted."""
    off, times = csr([10, 12, 14, 15, 19, 20])
    v = VM.verdicts_from_lists(off, times, 0, 100, lock=([INTERVAL], [3000], None, None), ttl_of=lambda r, t: 5)
    assert v.tolist() == [0, S, S, 0, S, 0]


def test_lock_alone_adds_the_run_time():
    """ALONE, avg 2500 ms (d = 3), ttl 5: 10 granted, free_at = 10 + 3 + 5 =
    18: 17 skipped, 18 granted.  A negative AvgTime counts as 0."""
    off, times = csr([10, 17, 18])
    v = VM.verdicts_from_lists(off, times, 0, 100, lock=([ALONE], [2500], None, None), ttl_of=lambda r, t: 5)
    assert v.tolist() == [0, S, 0]
    off, times = csr([10, 14, 15])
    v = VM.verdicts_from_lists(off, times, 0, 100, lock=([ALONE], [-7], None, None), ttl_of=lambda r, t: 5)
    assert v.tolist() == [0, S, 0]


def test_ttl_zero_is_skipped_and_leaves_the_state():
    """ttl 0 at t = 10: skipped, the key untouched, so 11 (ttl 3) is granted
    with free_at 14; 13 skipped; 14 has ttl 0: skipped although the key is
    gone; 15 granted."""
    ttl = {10: 0, 11: 3, 14: 0, 15: 3}
    off, times = csr([10, 11, 13, 14, 15])
    v = VM.verdicts_from_lists(off, times, 0, 100, lock=([INTERVAL], [0], None, None), ttl_of=lambda r, t: ttl[t])
    assert v.tolist() == [S, 0, S, S, 0]


def test_non_contending_rule_and_common_unit():
    """A job of three rules, rule 1 not contending: its fires get 0 and do not
    take the key.  Rules 0 and 2 share it: (10, rule 0) granted with ttl 4,
    (10, rule 2) and (12, rule 2) skipped, (14, rule 0) granted.  The COMMON
    unit (rule 3) gets 0 whatever fires."""
    off, times = csr([10, 14], [10, 11, 12], [10, 12], [10, 11])
    lock = ([ALONE, ALONE, ALONE, COMMON], [0, 0, 0, 9000], [7, 7, 7, 8], [1, 0, 1, 1])
    v = VM.verdicts_from_lists(off, times, 0, 100, lock=lock, ttl_of=lambda r, t: 4)
    assert v.tolist() == [0, 0, 0, 0, 0, S, S, 0, 0]


def test_both_bits_on_one_fire_and_independence():
    """One rule, fires 1..4; P = 1 with d = 2 drops 2 and 4; an INTERVAL lock
    with ttl 3 skips 2 and 3.  Fire 2 carries both bits, and each bit alone
    equals the call with only that argument: the processes are not composed."""
    off, times = csr([1, 2, 3, 4])
    admit = ([2000], [1], None)
    lock = ([INTERVAL], [0], None, None)
    both = VM.verdicts_from_lists(off, times, 0, 10, admit=admit, lock=lock, ttl_of=lambda r, t: 3)
    assert both.tolist() == [0, D | S, S, D]
    a = VM.verdicts_from_lists(off, times, 0, 10, admit=admit)
    s = VM.verdicts_from_lists(off, times, 0, 10, lock=lock, ttl_of=lambda r, t: 3)
    assert (a | s).tolist() == both.tolist() and a.tolist() == [0, D, 0, D] and s.tolist() == [0, S, S, 0]


def test_stuck_ttl_raises():
    off, times = csr([5])
    with pytest.raises(LockStuck):
        VM.verdicts_from_lists(off, times, 0, 10, lock=([ALONE], [0], None, None), ttl_of=lambda r, t: None)


def test_empty_and_select():
    off, times = csr([], [3, 4, 9], [], [4])
    v = np.array([D, 0, D | S, S], dtype=np.uint8)
    so, st = VM.select(off, times, v, 1, 1)
    assert so.tolist() == [0, 0, 2, 2, 2] and st.tolist() == [3, 9]
    so, st = VM.select(off, times, v, 3, 0)
    assert so.tolist() == [0, 0, 1, 1, 1] and st.tolist() == [4]
    so, st = VM.select(off, times, v, 2, 2)
    assert so.tolist() == [0, 0, 1, 1, 2] and st.tolist() == [9, 4]
    assert VM.first_diff(off, v, v) is None
    assert VM.first_diff(off, v, np.array([D, 0, D | S, 0], dtype=np.uint8)) == "rule 3 fire 0: 2 vs 0"
    off0, t0 = csr()
    assert VM.verdicts_from_lists(off0, t0, 0, 10, admit=([], [], None)).shape == (0,)
