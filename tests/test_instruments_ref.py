"""The host references of the device instruments (tests/instruments_ref.py):
the definition in Python integers against its numpy form, against
Engine.node_list_checksum (the host side of bench.py's every-step check),
against three known answers and the additivity the header promises.  The GPU
tests (tests/test_gpu_instruments.py) judge the kernels by these references."""
import numpy as np
import pytest

import instruments_ref as R
from instruments_ref import INT32_MAX, INT32_MIN, INT64_MAX, INT64_MIN, M64

FIRSTS = [0, (1 << 31) - 3, (1 << 32) - 3, 1 << 40, INT64_MAX - 2, -5]
ADDS = [0, 1, -1, INT64_MAX]


def arrays(seed, n=301):
    rng = np.random.default_rng(seed)
    v64 = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    v32 = rng.integers(INT32_MIN, INT32_MAX, n, dtype=np.int32, endpoint=True)
    v64[[0, 1, 7, n - 1]] = [INT64_MIN, -1, 0, INT64_MAX]
    v32[[0, 1, 7, n - 1]] = [INT32_MIN, -1, 0, INT32_MAX]
    return v64, v32


def test_known_answers():
    assert R.checksum_ref([0], 8) == 0
    assert R.checksum_ref([0, 1, 2], 8) == 0xcb5de655dc479cf9
    assert R.checksum_ref([-1, INT64_MIN, INT64_MAX], 8, first_index=INT64_MAX - 1, add=1) == 0x8b9e43e335c2d6ff
    # the same three through the numpy form, and an empty array
    assert R.checksum_ref_np(np.array([0], np.int64), 8) == 0
    assert R.checksum_ref_np(np.array([0, 1, 2], np.int64), 8) == 0xcb5de655dc479cf9
    assert R.checksum_ref_np(np.array([-1, INT64_MIN, INT64_MAX], np.int64), 8, INT64_MAX - 1, 1) == 0x8b9e43e335c2d6ff
    assert R.checksum_ref([], 8) == 0 and R.checksum_ref_np(np.empty(0, np.int32), 4, 5, 7) == 0


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("add", ADDS)
def test_bigint_equals_numpy(first, add):
    v64, v32 = arrays(1)
    assert R.checksum_ref(v64.tolist(), 8, first, add) == R.checksum_ref_np(v64, 8, first, add)
    assert R.checksum_ref(v32.tolist(), 4, first, add) == R.checksum_ref_np(v32, 4, first, add)


def test_int32_is_sign_extended():
    """An int32 array checksums as the int64 array of the same values, and not
    as its zero-extension."""
    _, v32 = arrays(2)
    assert R.checksum_ref_np(v32, 4, 9, -1) == R.checksum_ref_np(v32.astype(np.int64), 8, 9, -1)
    assert R.checksum_ref([-1], 4) == R.checksum_ref([-1], 8) != R.checksum_ref([0xFFFFFFFF], 8)
    # a 32-bit word given unsigned is the signed value it holds
    assert R.checksum_ref([0xFFFFFFFF], 4) == R.checksum_ref([-1], 4)


@pytest.mark.parametrize("elem_bytes", [8, 4])
@pytest.mark.parametrize("first", FIRSTS)
def test_additivity(elem_bytes, first):
    v = arrays(3)[0 if elem_bytes == 8 else 1]
    n = len(v)
    whole = R.checksum_ref(v.tolist(), elem_bytes, first, 1)
    assert whole == R.checksum_ref_np(v, elem_bytes, first, 1)
    for c in (0, 1, 64, 255, 256, n - 1, n):
        parts = R.checksum_ref(v[:c].tolist(), elem_bytes, first, 1) + R.checksum_ref(v[c:].tolist(), elem_bytes, first + c, 1)
        assert parts & M64 == whole, c
        parts = R.checksum_ref_np(v[:c], elem_bytes, first, 1) + R.checksum_ref_np(v[c:], elem_bytes, first + c, 1)
        assert parts & M64 == whole, c


def test_order_and_bits_matter():
    v = np.arange(10, 20, dtype=np.int64)
    base = R.checksum_ref_np(v, 8)
    w = v.copy()
    w[[3, 4]] = w[[4, 3]]
    assert R.checksum_ref_np(w, 8) != base
    for bit in (0, 31, 32, 40, 63):
        w = v.copy()
        w[5] ^= np.int64(1) << np.int64(bit) if bit < 63 else np.int64(INT64_MIN)
        assert R.checksum_ref_np(w, 8) != base, bit


def test_engine_node_list_checksum_equals_ref():
    """Engine.node_list_checksum (static numpy; what bench.py's every-step
    verification compares the device checksums with) against the reference."""
    from cronsun_amd.engine import Engine
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 63, 64, 65, 257, 1000):
        time = np.sort(rng.integers(1767225600, 1767225600 + 86400, n)).astype(np.int64)
        rule = rng.integers(0, 10_000_000, n).astype(np.int32)
        if n >= 2:
            time[0], time[-1] = INT64_MIN, INT64_MAX
            rule[0], rule[-1] = INT32_MIN, -1
        exp = R.node_list_checksum_ref(time.tolist(), rule.tolist())
        assert exp == R.node_list_checksum_ref_np(time, rule)
        assert Engine.node_list_checksum(time, rule) == exp, n
        # lists as bench.py passes them: any integer dtype, python lists
        assert Engine.node_list_checksum(time.tolist(), rule.astype(np.int64)) == exp, n


def test_ref_rejects_other_widths():
    with pytest.raises(ValueError):
        R.checksum_ref([1], 2)
    with pytest.raises(ValueError):
        R.checksum_ref_np(np.zeros(3, np.int64), 4)
