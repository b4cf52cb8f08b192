"""The host model of the in-flight profile (inflight_model.py) pinned on the
CPU: against a brute-force double loop over fires and buckets, against the
start profile (profile_model.bin_fires) through the four identities of the
definition, the peaks model, and one case by hand."""
import numpy as np
import pytest

import inflight_model as IM
import profile_cases as PC
import profile_model as PM


def brute(off, times, t0, w, B, dur_ms):
    """The definition read literally, in milliseconds and without the rounded
    d: a fire t in (t0, t0 + B*w] is running at edge e when it has started
    (t <= e) and not yet finished (e < t + ms / 1000)."""
    K = len(off) - 1
    out = np.zeros((K, B), dtype=np.int32)
    for r in range(K):
        ms = int(dur_ms[r])
        for b in range(B):
            e = t0 + (b + 1) * w
            for t in times[off[r]:off[r + 1]]:
                t = int(t)
                if t0 < t <= t0 + B * w and t <= e and e * 1000 < t * 1000 + ms:
                    out[r, b] += 1
    return out


@pytest.mark.parametrize("w,B", [(1, 40), (7, 30), (60, 5)])
def test_model_vs_brute_force(w, B):
    """22 rules of random sorted fire lists (one empty, one with a fire every
    second, fires beyond the horizon), every duration of the cycle."""
    rng = np.random.default_rng(w * 100 + B)
    t0, H = 1000, w * B
    lists = [np.sort(rng.choice(np.arange(t0 + 1, t0 + H + 50), int(rng.integers(0, min(H, 60))), replace=False))
             for _ in range(20)]
    lists += [np.zeros(0, dtype=np.int64), np.arange(t0 + 1, t0 + H + 1)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    times = np.concatenate(lists).astype(np.int64)
    cyc = IM.duration_cycle(w)
    dur = [cyc[(r + w) % len(cyc)] for r in range(len(lists))]
    got = IM.inflight_from_lists(off, times, t0, w, B, IM.seconds(dur))
    assert got.dtype == np.int32 and got.shape == (len(lists), B)
    assert np.array_equal(got, brute(off, times, t0, w, B, dur))
    assert got.any()


def test_seconds_round_up():
    assert IM.seconds([0, 1, 999, 1000, 1001, IM.INT64_MAX]).tolist() == [0, 1, 1, 1, 2, IM.INT64_MAX // 1000 + 1]


@pytest.mark.parametrize("w,B", [(60, 65), (20, 4096), (3599, 22)])
def test_identities_against_the_start_profile(w, B):
    """On the UTC base (600 rules, 610k fires): d = 0 a zero matrix, d = w the
    start matrix, d = m*w the sliding sum of m start buckets, d >= B*w the
    prefix sums."""
    base = PC.utc_base()
    starts = base.matrix(w, B)
    K = base.K

    def model(d):
        return IM.inflight_from_lists(base.off, base.times, base.t0, w, B, np.full(K, d, dtype=np.int64))
    assert not model(0).any()
    assert np.array_equal(model(w), starts)
    for m in (2, 3, 7):
        assert np.array_equal(model(m * w), IM.sliding_sum(starts, m))
    pre = np.cumsum(starts, axis=1, dtype=np.int64)
    assert np.array_equal(model(B * w), pre)
    assert np.array_equal(model(IM.INT64_MAX // 1000 + 1), pre)
    assert np.array_equal(IM.sliding_sum(starts, B), pre) and np.array_equal(IM.sliding_sum(starts, 1), starts)
    assert pre.max() < 2**31


def test_peaks_model():
    nodes = np.array([[0, 0, 0], [1, 5, 5], [7, 2, 7], [0, 0, 3]], dtype=np.int64)
    peak, bucket = IM.peaks(nodes)
    assert peak.tolist() == [0, 5, 7, 3] and bucket.tolist() == [0, 1, 0, 2]
    assert peak.dtype == np.int64 and bucket.dtype == np.int32
    assert [len(x) for x in IM.peaks(np.zeros((0, 4), dtype=np.int64))] == [0, 0]


def test_by_hand():
    """t0 = 100, three buckets of 10 s: edges 110, 120, 130.  One rule firing
    at 101, 110, 111, 125.
    d = 1 (1 ms .. 1000 ms): running at an edge only when started on it.
    d = 10 = w: the start profile.  d = 15: (95->100, 110], (105, 120], (115, 130]."""
    off, times = np.array([0, 4], dtype=np.int64), np.array([101, 110, 111, 125], dtype=np.int64)

    def row(ms):
        return IM.inflight_from_lists(off, times, 100, 10, 3, IM.seconds([ms]))[0].tolist()
    assert row(0) == [0, 0, 0]
    assert row(1) == row(1000) == [1, 0, 0]
    assert row(1001) == [1, 0, 0]  # d = 2: (108, 110], (118, 120], (128, 130]
    assert row(10_000) == PM.bin_fires(off, times, 100, 10, 3)[0].tolist() == [2, 1, 1]
    assert row(15_000) == [2, 2, 1]
    assert row(IM.INT64_MAX) == [2, 3, 4]
