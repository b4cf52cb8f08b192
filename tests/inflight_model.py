"""Host model of the in-flight profile (cg_inflight_*, cg_profile_node_peaks).

Plain numpy, no call into the library or the oracle.  With bucket edges e_b =
t0 + (b+1)*w and a duration of d whole seconds per rule (dur_ms / 1000 rounded
up), cell [r, b] counts the fires t of rule r in (t0, t0 + B*w] with
max(t0, e_b - min(d, B*w)) < t <= e_b: two ranks in the rule's sorted fire
list.  test_inflight_model.py pins it to a brute-force double loop and to the
start profile (profile_model.bin_fires) through the identities; the GPU tests
hold the kernels to it.
"""
import numpy as np

INT64_MAX = (1 << 63) - 1


def seconds(dur_ms):
    """int64 [R]: dur_ms / 1000 rounded up (no overflow at INT64_MAX)."""
    d = np.asarray(dur_ms, dtype=np.int64)
    return d // 1000 + (d % 1000 != 0)


def inflight_from_lists(off, times, t0, w, B, d_sec):
    """int32 [K, B] from a CSR of sorted fire lists (off [K+1], times in
    (t0, ...]; fires past t0 + B*w are never counted since e_b <= t0 + B*w)."""
    K = len(off) - 1
    times = np.asarray(times, dtype=np.int64)
    e = t0 + (np.arange(B, dtype=np.int64) + 1) * w
    out = np.zeros((K, B), dtype=np.int32)
    for r in range(K):
        ts = times[off[r]:off[r + 1]]
        lo = np.maximum(t0, e - min(int(d_sec[r]), B * w))
        out[r] = np.searchsorted(ts, e, "right") - np.searchsorted(ts, lo, "right")
    return out


def sliding_sum(starts, m):
    """int64 [K, B]: cell b = the sum of start buckets b-m+1 .. b (those >= 0)."""
    run = np.zeros((starts.shape[0], starts.shape[1] + 1), dtype=np.int64)
    np.cumsum(starts, axis=1, dtype=np.int64, out=run[:, 1:])
    b = np.arange(starts.shape[1])
    return run[:, b + 1] - run[:, np.maximum(b + 1 - m, 0)]


def peaks(nodes):
    """(int64 [N] largest cell, int32 [N] first bucket attaining it) per row;
    a zero row gives (0, 0)."""
    if nodes.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    return nodes.max(axis=1).astype(np.int64), nodes.argmax(axis=1).astype(np.int32)


def duration_cycle(w, B=None):
    """The durations (ms) the tests cycle through by rule index: around one
    second, around the width, 3.5 widths, 45 days, and INT64_MAX."""
    return [0, 1, 999, 1000, 1001, w * 1000 - 1, w * 1000, w * 1000 + 1, 3500 * w, 45 * 86400 * 1000, INT64_MAX]
